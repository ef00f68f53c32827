"""The dispatch records' layout (csrc/rt_blob.h RtTileRec; k_masks.hip tile_records_kernel writes entry e's
record at records[e], rt_device.h rows_entry reads it there): a host mirror of the gather checks that every
entry of a launch gets exactly one record holding its own tile's first pixel and mask words, for orders that
are permutations and for the identity; the record's shape and the option constant are read from the headers."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinyraytracerinrust_amd", "csrc")


def _words():
    text = open(os.path.join(CSRC, "rt_blob.h")).read()
    assert re.search(r"struct alignas\(32\) RtTileRec \{\s*int32_t x0, r0;[^\n]*\n\s*uint32_t mask\[RT_TILEMASK_WORDS\];\s*\};", text)
    return int(re.search(r"#define RT_TILEMASK_WORDS (\d+)", text).group(1))


def _gather(order, masks, tiles_x):
    """tile_records_kernel on the host: records [entries, 2 + words] (x0, r0, mask words)."""
    table = np.full((len(order), 2 + masks.shape[1]), -1, dtype=np.int64)
    for e, tile in enumerate(order):
        table[e, 0] = (tile % tiles_x) * 8
        table[e, 1] = (tile // tiles_x) * 8
        table[e, 2:] = masks[tile] if tile < len(masks) else 0xffffffff
    return table


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2115])
@pytest.mark.parametrize("identity", [False, True])
def test_every_entry_reads_its_own_tile(n, identity):
    words = _words()
    assert 4 * (2 + words) == 32                        # one record: a 32-byte scalar load
    rng = np.random.default_rng(n)
    order = np.arange(n) if identity else rng.permutation(n)
    masks = rng.integers(0, 2**32, size=(n, words), dtype=np.int64)
    tiles_x = 47 if n == 2115 else max(1, min(n, 3))
    table = _gather(order, masks, tiles_x)
    # workgroup e of the launch renders order[e]: the pixels of its record are that tile's, each tile once
    tiles = (table[:, 1] // 8) * tiles_x + table[:, 0] // 8
    assert (tiles == order).all() and sorted(tiles) == list(range(n))
    assert (table[:, 0] < tiles_x * 8).all() and (table[:, 2:] == masks[order]).all()


def test_kernel_and_gather_agree_on_the_slot():
    """Writer and reader index the table by the order entry alone."""
    assert "out[e] = r;" in open(os.path.join(CSRC, "k_masks.hip")).read()
    assert "as_const(recs) + entry;" in open(os.path.join(CSRC, "rt_bodies.h")).read()   # rows_entry


def test_option_constant_and_header_agree():
    from tinyraytracerinrust_amd import _lib
    assert _lib.RT_OPT_TILE_RECORDS == 10
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    assert "RT_OPT_TILE_RECORDS = 10" in header
