"""The sample programs (tinyraytracerinrust_amd/csrc/spec_text.cpp rt_spec_points / rt_spec_aa, RT_OPT_SPEC_SAMPLES)
on the CPU: the ABI's new symbols, and the two kernels hipRTC builds for a scene without a device
(rt_scene_sample_report), inside the resource guard's bounds of the scene's mode -- while the row programs
stay the three that rt_scene_spec_report names.  What they render is checked on the GPU
(tests/test_gpu_spec_samples.py)."""
import ctypes
import inspect

from tests.conftest import SCENES, scene_text

MAX_VGPRS, MAX_SCRATCH_ROWS = 128, 1024       # spec_compile.cpp RT_SPEC_MAX_VGPRS, RT_SPEC_MAX_SCRATCH_ROWS (reflection, chain)


def _lines(report):
    out = {}
    for line in report.splitlines():
        if line.startswith("compiler: "):
            continue
        name, rest = line.split(": ", 1)
        f = rest.split()
        out[name] = {f[i]: f[i + 1] for i in range(0, len(f) - 1, 2)}
    return out


def test_new_symbols_and_arity():
    import tinyraytracerinrust_amd as T
    from tinyraytracerinrust_amd import _lib
    assert _lib.RT_OPT_SPEC_SAMPLES == 9
    L = T.lib()
    want = {"rt_ctx_spec_wait_samples": (ctypes.c_int, 2), "rt_ctx_sample_kernel_info": (ctypes.c_int, 3),
            "rt_scene_sample_report": (ctypes.c_int, 4)}
    for name, (res, n) in want.items():
        fn = getattr(L, name)                              # exported by the library
        sig = _lib.SIGNATURES[name]
        assert sig[0] is res and len(sig[1]) == n and fn.restype is res and len(fn.argtypes) == n, name
    with open(_lib.HERE + "/../include/rt_abi.h") as f:
        header = f.read()
    assert "RT_OPT_SPEC_SAMPLES = 9" in header
    assert "int rt_ctx_spec_wait_samples(rt_ctx* ctx, int32_t timeout_ms);" in header
    assert "int rt_ctx_sample_kernel_info(rt_ctx* ctx, char* buf, size_t cap);" in header
    assert "int rt_scene_sample_report(const rt_scene* scene, char* buf, size_t cap, size_t* len);" in header
    for cls, names in ((T.Renderer, ("spec_wait_samples", "sample_kernel_info", "set_spec_samples")),
                       (T.Scene, ("sample_report",))):
        for n in names:
            assert inspect.isfunction(getattr(cls, n)), n


def test_sample_report_lists_the_two_kernels_within_the_guard():
    import tinyraytracerinrust_amd as T
    for text in ("draw(sphere(<0,0,0>,30,red))", scene_text("globes")):
        s = T.Scene.compile(text, 0.0, 64, 48, asset_dir=SCENES)
        assert s.status == 0, s.error
        report = s.sample_report()
        ks = _lines(report)
        assert list(ks) == ["rt_spec_points", "rt_spec_aa"], report
        for name, v in ks.items():                         # both scenes are reflection-only: the row kernel's bounds
            assert 0 < int(v["vgprs"]) <= MAX_VGPRS and 0 <= int(v["scratch"]) <= MAX_SCRATCH_ROWS, (name, v)
            assert v["source"] in ("hiprtc", "disk")


def test_row_programs_are_still_the_three():
    import tinyraytracerinrust_amd as T
    s = T.Scene.compile(scene_text("globes"), 0.0, 64, 48, asset_dir=SCENES)
    s.sample_report()                                      # the sample programs are in the process now
    ks = _lines(s.spec_report())
    assert set(ks) == {"rt_spec_rows_00", "rt_spec_def_00", "rt_spec_prim_00"}, ks
    prog = s.spec_program()
    assert "rt_spec_points" not in prog and "rt_spec_aa" not in prog
