// rt_bodies.h -- the last part of the device core (rt_device.h; after rt_trace.h): the scene's device view
// from a kernel's arguments (make_ds), camera rays, tile and band indexing, pixel stores, and the bodies
// the kernels wrap -- rows_entry / rows_body, rows_views_body, points_body, aa_trace_body, deferred_body.
#pragma once

namespace {

// RT_SPEC: every table is the scene's constexpr copy (spec_text.cpp), only the texels stay in HBM;
// RT_SPEC_FAMILY: the family's constexpr tables plus this scene's own (RT_REC).
__device__ __forceinline__ DS make_ds(const RtDevScene& s) {
  DS d;
#ifdef RT_SPEC
#ifdef RT_SPEC_FAMILY
  // the merged tables (RT_REC) read this scene's own; nodes, programs and textures are the family's
  d.objects = as_const(s.objects);
  d.trav = as_const(s.trav);
  d.strav = as_const(s.strav);
  d.leaves = as_const(s.leaves);
  d.lights = as_const(s.lights);
#else
  d.objects = as_const(rt_spec::OBJECTS);
  d.trav = as_const(rt_spec::TRAV);
  d.strav = as_const(rt_spec::STRAV);
  d.leaves = as_const(rt_spec::LEAVES);
  d.lights = as_const(rt_spec::LIGHTS);
#endif
  d.n_trav = rt_spec::N_TRAV;
  d.n_strav = rt_spec::N_STRAV;
  d.nodes = as_const(rt_spec::NODES);
  d.prog = as_const(rt_spec::PROG);
  d.textures = as_const(rt_spec::TEXTURES);
  d.n_objects = rt_spec::N_OBJECTS;
  d.n_lights = rt_spec::N_LIGHTS;
  d.shadow_early_out = rt_spec::SHADOW_EARLY_OUT;
#else
  d.objects = as_const(s.objects);
  d.trav = as_const(s.trav);
  d.n_trav = s.n_trav;
  d.strav = as_const(s.strav);
  d.n_strav = s.n_strav;
  d.trav_c = as_const(s.trav_c);
  d.strav_c = as_const(s.strav_c);
  d.nodes = as_const(s.nodes);
  d.leaves = as_const(s.leaves);
  d.prog = as_const(s.prog);
  d.lights = as_const(s.lights);
  d.textures = as_const(s.textures);
  d.n_objects = s.n_objects;
  d.n_lights = s.n_lights;
  d.shadow_early_out = s.shadow_early_out;
#endif
  d.texels = s.texels;
  return d;
}

// PerspectiveCamera::create_ray (camera.rs:65-74)
__device__ __forceinline__ void camera_ray(const RtCamera& cam, double x, double y, V3* ro, V3* rd) {
  double sx = ((x / cam.width) - 0.5) * cam.aspect;
  double sy = (cam.height - 1.0 - y) / cam.height - 0.5;
  *rd = add(add(ld3(cam.direction), scale(ld3(cam.right), sx)), scale(ld3(cam.up), sy));
  *ro = ld3(cam.center);
}

// The same ray for an integer pixel (x, y) in the frame: the two divisions and their terms read from
// the upload's per-column / per-row tables (RtDevScene::cam_sx / cam_sy, computed by the host with
// camera_ray's expressions), the rest as camera_ray.
__device__ __forceinline__ void camera_ray_px(const RtDevScene& S, int x, int y, V3* ro, V3* rd) {
  const double sx = S.cam_sx[x], sy = S.cam_sy[y];
  *rd = add(add(ld3(S.cam.direction), scale(ld3(S.cam.right), sx)), scale(ld3(S.cam.up), sy));
  *ro = ld3(S.cam.center);
}

// Output rows r = 0 .. n_rows-1 of a band layout: r -> full-frame row
//   y = y_first + (r / band_rows) * band_pitch + r % band_rows
// (a contiguous tile [y0, y1) is one band; the cyclic multi-GPU layout deals bands of
// band_rows rows with pitch world * band_rows).
// Kernel modes (RT_MODE_*): the reflection-only megakernel; refraction scenes whose rays form
// chains (RtDevScene::ray_chains: frames are (A, w) only, no pending-reflection state); refraction
// scenes with ray trees.  Each mode's waves per SIMD: rt_tunables.h.
#define RT_WAVES(REFR) ((REFR) ? RT_WAVES_PER_EU : RT_WAVES_PER_EU_NOREFR)
#define RT_WAVES_MODE(M) ((M) == RT_MODE_REFL ? RT_WAVES_PER_EU_NOREFR : (M) == RT_MODE_CHAIN ? RT_WAVES_PER_EU_CHAIN : RT_WAVES_PER_EU)
// Workgroup = one wave of 8x8 pixels: measured 3-5 % faster than 2x2-wave workgroups (round 1).
constexpr int RT_WG_THREADS = 64;
// Tile = the 64 pixels of one wave, RT_TILE_W x RT_TILE_H (RT_TILE_W in rt_blob.h).  Pixel `pix` of tile `tile` -> (x, output row r).
constexpr int RT_TILE_H = 64 / RT_TILE_W;
static_assert(RT_TILE_W * RT_TILE_H == 64, "a tile is one wave's 64 pixels");
__device__ __forceinline__ void tile_pixel(unsigned tile, int pix, int width, int* x, int* r) {
  const unsigned tiles_x = (unsigned)(width + RT_TILE_W - 1) / RT_TILE_W;
  *x = (int)(tile % tiles_x) * RT_TILE_W + pix % RT_TILE_W;
  *r = (int)(tile / tiles_x) * RT_TILE_H + pix / RT_TILE_W;
}
// The frame-sized side kernels (k_aa.hip classify and edges, k_ortho.hip) take 16x16 tiles, row-major over `width`:
// a workgroup of four waves, wave w the 8x8 quadrant (w & 1, w >> 1).  Thread `thread` of workgroup `block` -> (x, r).
__device__ __forceinline__ void tile16_pixel(unsigned block, unsigned thread, int width, int* x, int* r) {
  const int lane = thread & 63, wave = thread >> 6;
  const int tiles_x = (width + 15) >> 4;
  *x = ((block % tiles_x) << 4) + ((wave & 1) << 3) + (lane & 7);
  *r = ((block / tiles_x) << 4) + ((wave >> 1) << 3) + (lane >> 3);
}

// Output row r of a launch -> its frame row (see above); a launch of one band (every single-GPU frame)
// skips the per-lane integer division and remainder (a wave-uniform branch).
__device__ __forceinline__ int band_row(int r, int y_first, int band_rows, int band_pitch, int n_rows) {
  if (band_rows >= n_rows) return y_first + r;
  return y_first + (r / band_rows) * band_pitch + r % band_rows;
}

// One pixel's colour into an output row: f64 RGBA (alpha 1 after any colour op), packed RGB8 (band
// gathers) or RGBA8 with `(c * 255.0) as u8` per channel (easy_pixbuf.rs:46-53).
// The RGBA8 / RGB8 frame is written once and read by another kernel or the host: nontemporal
// (streaming) stores.  A wave's 8x8 tile covers a quarter of eight 128-byte lines and the tiles
// sharing a line run at different times on different XCDs, so through the L2s every row segment
// reached memory as its own partial-line write-back.
// PLAIN: write-back stores (the primary-ray kernels, below).
template <bool PLAIN = false, class T>
__device__ __forceinline__ void frame_store(T v, T* p) {
  if constexpr (PLAIN) *p = v;
  else __builtin_nontemporal_store(v, p);
}
template <bool F64, bool PLAIN = false>
__device__ __forceinline__ void store_pixel(uint8_t* row, int x, Col c, int rgb) {
  if constexpr (F64) {
    double* o = (double*)row + (size_t)x * 4;
    o[0] = c.r; o[1] = c.g; o[2] = c.b; o[3] = 1.0;
  } else if (rgb) {
    uint8_t* o = row + (size_t)x * 3;
    frame_store<PLAIN>((uint8_t)to_u8(c.r), o);
    frame_store<PLAIN>((uint8_t)to_u8(c.g), o + 1);
    frame_store<PLAIN>((uint8_t)to_u8(c.b), o + 2);
  } else {
    frame_store<PLAIN>(to_u8(c.r) | (to_u8(c.g) << 8) | (to_u8(c.b) << 16) | (255u << 24), (uint32_t*)row + x);
  }
}
// The side kernels' pixel, with an alpha of its own (k_aa.hip, k_ortho.hip): into row `row` of an RGBA8 plane
// and of an f64 plane, each optional (null) with its stride in bytes; plain stores.
__device__ __forceinline__ void put_rgba(double r, double g, double b, double a, int x, int row, uint8_t* u8,
                                         size_t u8_stride, double* f64, size_t f64_stride) {
  if (u8) ((uint32_t*)(u8 + (size_t)row * u8_stride))[x] = to_u8(r) | (to_u8(g) << 8) | (to_u8(b) << 16) | (to_u8(a) << 24);
  if (f64) {
    double* o = (double*)((uint8_t*)f64 + (size_t)row * f64_stride) + (size_t)x * 4;
    o[0] = r; o[1] = g; o[2] = b; o[3] = a;
  }
}

// ---------------------------------------------------------------- kernel bodies
// The row kernels' bodies, shared by the generic kernels (k_rows.hip) and the scene-specialised ones
// (spec_text.cpp).  Output rows r = 0 .. n_rows-1 of a band layout; wave = one 8x8 tile.
// Tile dispatch order (see launch_bands): `order` lists the tiles most expensive first, as measured
// on a calibration launch that stored each tile's wave time in `cost`.  CAL (the calibration
// instantiation) is the only one that carries the timing code.
// KL_ >= 0: that many stack frames in LDS (the specialised kernels at 4 waves/SIMD have room for more).
// rows_entry: entry `entry` of the launch (a tile index, or the order's entry-th tile); rows_body: the
// workgroup's own entry (blockIdx.x).  (A wave looping over several entries grid-stride was measured
// and lost: the loop's live state cost the megakernels 6 more spilled VGPRs, profiles/r07c_tiles_per_wave.txt.)
// The row kernels' frame storage per one-wave workgroup: the chain mode takes a wave pool (trace(), KP
// slots) and the reflection-only mode per-lane frames by default (RT_LDS_POOL_* / RT_LDS_FRAMES*,
// rt_tunables.h); KL_ >= 0 asks for KL_ frames per lane instead, KP_ >= 0 sets the pool's size (A/B
// instantiations).  The ray-tree mode keeps per-lane frames.
template <int MODE, int KL_ = -1, int KP_ = -1>
constexpr int rows_pool_slots() {
  return MODE == RT_MODE_TREE ? 0 : KP_ >= 0 ? KP_ : MODE == RT_MODE_CHAIN ? RT_LDS_POOL_CHAIN : RT_LDS_POOL_REFL;
}
template <int MODE, int KL_ = -1>
constexpr int rows_lane_frames() {
  return KL_ >= 0 ? KL_ : MODE == RT_MODE_CHAIN ? RT_LDS_FRAMES_CHAIN : RT_LDS_FRAMES;
}
// PRIM (the primary-ray kernels of the specialised programs, launches with max_depth 0): max_depth is the
// compile-time 0, so trace() never pushes a frame -- no frame stack, no LDS, no bounce loop -- and the
// frame takes write-back stores (such launches order their tiles by 128-byte line and XCD, k_rows.hip
// xcd_line_order, so a line's four tiles are written back to back through one L2).
template <int MODE, bool F64, bool CAL, bool FC, int KL_ = -1, int KP_ = -1, bool PRIM = false>
__device__ __forceinline__ void rows_entry(const RtDevScene& S, unsigned entry, int y_first, int band_rows, int band_pitch,
                                           int n_rows, int max_depth, uint8_t* __restrict__ out, size_t stride,
                                           const int32_t* __restrict__ order, uint32_t* __restrict__ cost, int rgb,
                                           lds_f64* frames, const uint32_t* __restrict__ masks = nullptr,
                                           const RtTileRec* __restrict__ recs = nullptr) {
  constexpr bool REFR = MODE != RT_MODE_REFL, CHAIN = MODE == RT_MODE_CHAIN;
  constexpr int KLR = PRIM ? 0 : MODE == RT_MODE_TREE ? RT_LDS_RFRAMES : 0;
  constexpr int KP = PRIM ? 0 : rows_pool_slots<MODE, KL_, KP_>();
  constexpr int KL = PRIM ? 0 : rows_lane_frames<MODE, KL_>();
  if constexpr (PRIM) max_depth = 0;
  const int lane = threadIdx.x & 63;
  [[maybe_unused]] uint64_t t_start = 0;
  if constexpr (CAL) t_start = wall_clock64();
#if defined(RT_SPEC) && RT_TILE_MASKS
  // The masked single-scene kernels: every kernel argument the prologue and the final store read is asked for
  // here, so the compiler issues their loads together at entry, behind ONE wait (left to itself it sinks each
  // load into the block of its first use: four dependent trips before the first camera-table load, and one
  // for out / stride behind the whole trace).  No instruction; the values are wave-uniform scalars.
  if constexpr (MODE == RT_MODE_REFL)
    asm volatile("" ::"s"(recs), "s"(masks), "s"(order), "s"(S.width), "s"(S.height), "s"(n_rows), "s"(y_first),
                 "s"(band_rows), "s"(band_pitch), "s"(S.cam_sx), "s"(S.cam_sy), "s"(out), "s"(stride), "s"(rgb),
                 "s"(S.cam.center[0]), "s"(S.cam.center[1]), "s"(S.cam.center[2]), "s"(S.cam.direction[0]),
                 "s"(S.cam.direction[1]), "s"(S.cam.direction[2]), "s"(S.cam.right[0]), "s"(S.cam.right[1]),
                 "s"(S.cam.right[2]), "s"(S.cam.up[0]), "s"(S.cam.up[1]), "s"(S.cam.up[2]));
#endif
  unsigned tile;
  int x, r;
  TileMask tm = tile_mask_ones();
  if (recs) {
    // The entry's dispatch record (rt_blob.h RtTileRec): one 32-byte scalar load at an address made of a kernel
    // argument and the workgroup id -- the tile's first pixel (no order entry, no division) and its mask
    // words.  The records hold the launch's order; a calibrating launch has none (entry e is tile e).
    const cptr<RtTileRec> R = as_const(recs) + entry;
    tile = entry;
#if defined(RT_SPEC) && RT_TILE_MASKS
    // A lean tile (RT_OPT_LEAN_TILES; lean_body below): the record's x0 carries the sign bit, and the lean kernel
    // launched ahead of this one renders the entry.  At kernel entry, next to the sky branch; not in the
    // calibrating kernels (cost[tile] stays a tile's full time) nor the primary-ray kernel, whose launches'
    // tables never carry the bit (launch_plan.h).
    if constexpr (rt_spec::LEAN_OK && !CAL && !PRIM && MODE == RT_MODE_REFL)
      if (R->x0 < 0) return;
#endif
    int r0 = R->r0;
#if defined(RT_SPEC) && RT_TILE_MASKS
    // An entry traced for every hit (RT_OPT_TRACED_MASKS 1 / 3; trace_masks_body `objects`): the record's r0 carries
    // the sign bit, one scalar more for trace().  Only this kernel's tables carry it, as with the lean bit above.
    if constexpr (rt_spec::LEAN_OK && !CAL && !PRIM && MODE == RT_MODE_REFL) {
      tm.hit_min = r0 < 0 ? 0x7fffffff : 0;
      r0 &= 0x7fffffff;
    }
#endif
    x = R->x0 + lane % RT_TILE_W;
    r = r0 + lane / RT_TILE_W;
    for (int k = 0; k < RT_TILEMASK_WORDS; ++k) tm.w[k] = R->mask[k];
#if defined(RT_SPEC) && RT_TILE_MASKS
    // A sky tile (RT_OPT_SKY_FILL): the record's prim word is empty -- no boxed object in the tile's cone, and
    // the mask plane's own bit cleared because no ray of the tile can meet it; SKY_OK: the scene has no other
    // unbounded object -- so every valid pixel is BLACK (Color::BLACK, alpha as store_pixel writes it).  The
    // same guards and store as below; no camera-table load, no trace.  At kernel entry, not around the walks.
    // The calibrating kernels render every tile (cost[tile] stays a tile's full time).
    if constexpr (rt_spec::SKY_OK && !CAL)
      if (tm.w[0] == 0) {
        if (x >= S.width || r >= n_rows) return;
        if (band_row(r, y_first, band_rows, band_pitch, n_rows) >= S.height) return;
        store_pixel<F64, PRIM>(out + (size_t)r * stride, x, Col{0.0, 0.0, 0.0}, rgb);
        return;
      }
#endif
  } else {
    tile = CAL || !order ? entry : (unsigned)order[entry];
    tile_pixel(tile, lane, S.width, &x, &r);
    if (masks) {                            // the tile's row of the mask table; the tile index is the same in every lane
      const cptr<uint32_t> tw = as_const(masks) + (size_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)tile) * RT_TILEMASK_WORDS;
      for (int k = 0; k < RT_TILEMASK_WORDS; ++k) tm.w[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)tw[k]);
    }
  }
  if (x >= S.width || r >= n_rows) return;
  const int y = band_row(r, y_first, band_rows, band_pitch, n_rows);
  if (y >= S.height) return;
  V3 ro, rd;
  camera_ray_px(S, x, y, &ro, &rd);                                         // get_pixel(x as f64, y as f64)
  const Col c = trace<REFR, NoRec, KL, FC, KLR, CHAIN, KP>(make_ds(S), ro, rd, max_depth, nullptr, PRIM ? nullptr : frames + lane,
                                                         frames, tm);
  store_pixel<F64, PRIM>(out + (size_t)r * stride, x, c, rgb);
  if constexpr (CAL)
    if (threadIdx.x == 0) cost[tile] = (uint32_t)(wall_clock64() - t_start);   // vector store
}
template <int MODE, bool F64, bool CAL, bool FC, int KL_ = -1, int KP_ = -1, bool PRIM = false>
__device__ __forceinline__ void rows_body(const RtDevScene& S, int y_first, int band_rows, int band_pitch, int n_rows,
                                          int max_depth, uint8_t* __restrict__ out, size_t stride,
                                          const int32_t* __restrict__ order, uint32_t* __restrict__ cost, int rgb,
                                          lds_f64* frames, const uint32_t* __restrict__ masks = nullptr,
                                          const RtTileRec* __restrict__ recs = nullptr) {
  rows_entry<MODE, F64, CAL, FC, KL_, KP_, PRIM>(S, blockIdx.x, y_first, band_rows, band_pitch, n_rows, max_depth, out,
                                                 stride, order, cost, rgb, frames, masks, recs);
}
#if defined(RT_SPEC) && RT_TILE_MASKS
// Lean tiles (RT_OPT_LEAN_TILES; DESIGN.md "Lean tiles"): an entry whose prim word, the shadow words of the scene's
// lights and refl word hold no object but the mask plane, in a scene whose every other object is boxed
// (rt_spec::LEAN_OK).  Every walk of such a tile up to the depth-1 nearest hit visits the plane alone, exactly as
// under a mask of 0, so a pixel is trace<false>'s first iteration with that mask -- the plane hit, its lights
// (hit_lights), the inside test -- and its reflected ray, the same functions inlined on the same values: the
// same bits.  The reflected ray starts ON the plane and the plane's own leaf test still runs on it; whether it
// ever accepts a hit is not argued from rounding but CHECKED: lean_check_body runs this function's CHECK form
// (no lights, no store; the depth-1 walk kept) over the candidate entries once per record table and clears the
// bit of any entry in which a lane's reflected ray hits.  In the entries that keep it the ray misses, its
// colour is BLACK, and the render form folds the one frame as trace() does without walking.
// CHECK: true when the pixel's reflected ray hits something.
template <bool FC, bool CHECK>
__device__ __forceinline__ bool lean_pixel(const DS& ds, V3 ro, V3 rd, int max_depth, Col* C) {
  constexpr bool SHARE = false, OBB = true;                                // trace<false>'s walks
  double t_hit;
  const int oi = nearest_hit<SHARE, OBB>(ds, ro, rd, &t_hit, 0u);
  *C = {0.0, 0.0, 0.0};                                                    // Color::BLACK
  if (oi < 0) return false;
  const V3 p = add(ro, scale(rd, t_hit));
  V3 nrm = {0.0, 0.0, 0.0};
  Col c = {0.0, 0.0, 0.0}, L = {0.0, 0.0, 0.0};
  double transp = 0.0, refl = 0.0, nlen = 0.0;
  if constexpr (CHECK) shade_inputs(ds, oi, p, &nrm, &c, &transp, &refl, &nlen);
  else L = hit_lights<FC, SHARE, OBB>(ds, oi, p, 0u, &nrm, &c, &transp, &refl, &nlen);
  // trace<false> at depth 0: rp = refl, a reflection where depth < max_depth, rp != 0 and the hit is seen from outside
  const bool spawn = max_depth > 0 && refl != 0.0 && !hit_inside(rd, nrm, nlen);
  if (!spawn) {
    *C = L;
    return false;
  }
  if constexpr (CHECK) {
    double t1;
    return nearest_hit<SHARE, OBB>(ds, p, reflect_dir(rd, nrm), &t1, 0u) >= 0;
  }
  *C = cadd<FC>(intensify<FC>(L, 1.0 - refl), intensify<FC>(Col{0.0, 0.0, 0.0}, refl));   // the frame, folded with BLACK
  return false;
}
// The lean kernel's body: the megakernel's record load, guards, band_row and store over the same grid; an
// entry that is not lean returns at once (the megakernel renders it).
template <bool F64, bool FC>
__device__ __forceinline__ void lean_body(const RtDevScene& S, int y_first, int band_rows, int band_pitch, int n_rows,
                                          int max_depth, uint8_t* __restrict__ out, size_t stride, int rgb,
                                          const RtTileRec* __restrict__ recs) {
  const int lane = threadIdx.x & 63;
  const cptr<RtTileRec> R = as_const(recs) + blockIdx.x;
  const int x0 = R->x0;
  if (x0 >= 0) return;
  const int x = (x0 & 0x7fffffff) + lane % RT_TILE_W, r = R->r0 + lane / RT_TILE_W;
  if (x >= S.width || r >= n_rows) return;
  const int y = band_row(r, y_first, band_rows, band_pitch, n_rows);
  if (y >= S.height) return;
  V3 ro, rd;
  camera_ray_px(S, x, y, &ro, &rd);
  Col c;
  lean_pixel<FC, false>(make_ds(S), ro, rd, max_depth, &c);
  store_pixel<F64>(out + (size_t)r * stride, x, c, rgb);
}
// Traced tile masks (RT_OPT_TRACED_MASKS; DESIGN.md "Traced tile masks"): the predicate's words (rt_tilemask.h) hold
// for every ray of a tile's cone, the row kernels trace the pixel centres alone.  trace_masks_body runs once per
// record table, one wave per entry that is not sky already, traces the entry's own pixels with the functions
// trace<false> inlines -- camera_ray_px, nearest_hit, shade_inputs, hit_inside, reflect_dir, shadow_transparency on
// the same camera tables and the same record -- and keeps in each word only the objects whose tests accept a
// hit for some pixel of the entry, each word ANDed with what the record held:
//   prim       the walk runs under the record's prim word; the new word is the OR over the valid lanes of
//              1 << oi, the plane's bit included; empty: every pixel misses, the entry is sky (keep_bit: the bit
//              an empty word gets where no record may say sky, as the gather has it).  A walk over a subset that
//              holds each lane's winner returns that winner: the running best is the first object in walk order
//              that attains the minimum, and a subset keeps the relative order.
//   An entry in which a lane hits a boxed object stops here unless `objects` (below): the kernels read its other
//   words under all ones (trace(): plane_tile is false), so they stay the predicate's.  Else every hit is on the
//   mask plane, and
//   shadow[l]  for each boxed object o of the record's word the shadow walk runs under the one-bit mask 1 << o (the
//              plane ignores masks and is always walked); bit o stays where some lane's result for that walk
//              alone is 0.  These programs hold no transparent object (LEAN_OK), so the shadow product is
//              any-hit, and a shadow walk culls by the segment alone, never by another object's result: the
//              walk under the new word returns every lane what the walk under the old one did;
//   refl       the lanes that spawn a ray (refl != 0, seen from outside) trace it under the record's refl word; the
//              new word is the OR of 1 << oi over them, the plane's bit included (prim's argument); lanes that
//              spawn nothing contribute nothing.
// objects (RT_OPT_TRACED_MASKS 1 and 3): an entry with a pixel on a boxed object is traced too, with every lane that
// hit anything, plane or object -- the lanes trace() carries past `if (oi >= 0)`.  The predicate's shadow and refl
// words are made for hits on the mask plane (an object's far side is occluded by the object itself, whether or
// not its box shadows the floor under the tile), so here they are neither the candidates nor ANDed in: a shadow
// word's candidates are all boxed objects of the scene -- one walk under all of them first, and the one-bit walks
// only where some lane's result is 0 -- and the depth-1 ray is traced under all ones.  The entry's r0 then gets
// the sign bit (RtTileRec): its words 1..5 hold for every depth-0 hit, and trace() reads them as it does a floor
// tile's.  The arguments are the ones above; sky and lean entries come out the same either way.
// Lane exits mirror trace()'s, so each walk runs with the lanes it has there.  The first lane left writes the
// words (vector stores) and the lean bit of x0 where lean_on: prim is the plane alone, no shadow word of the
// scene's lights holds a boxed bit, refl is empty -- lean_check_body's own condition (no reflected ray accepts
// any hit, the plane's included), reached here without its candidates' detour through the predicate.
// Exactness is not argued from rounding: check and render call the same inlined functions on the same values, so
// a hit point here is the render's bit for bit.  The words hold for this table's pixel centres only (a table
// is keyed by the mask fill and the order it was gathered from, and by this option); they do not depend on
// max_depth (a refl word is read only where a depth-1 ray exists), on the output format or on FC (no colour is
// formed).
template <bool FC>
__device__ __forceinline__ void trace_masks_body(const RtDevScene& S, int y_first, int band_rows, int band_pitch, int n_rows,
                                                 RtTileRec* __restrict__ recs, bool lean_on, uint32_t keep_bit,
                                                 bool objects = false) {
  constexpr bool SHARE = false, OBB = true;                                // trace<false>'s walks
  constexpr int plane = rt_spec::MASK_PLANE;
  constexpr uint32_t plane_bit = plane >= 0 ? 1u << (plane & 31) : 0u;
  constexpr uint32_t boxed = spec_boxed_bits<true>(0, rt_spec::N_STRAV);
  const int lane = threadIdx.x & 63;
  RtTileRec* const R = recs + blockIdx.x;
  uint32_t w[RT_TILEMASK_WORDS];
  for (int k = 0; k < RT_TILEMASK_WORDS; ++k) w[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)R->mask[k]);
  const int x0 = __builtin_amdgcn_readfirstlane(R->x0) & 0x7fffffff, r0 = __builtin_amdgcn_readfirstlane(R->r0) & 0x7fffffff;
  if (w[0] == 0) return;                                                   // sky already
  const int x = x0 + lane % RT_TILE_W, r = r0 + lane / RT_TILE_W;
  if (x >= S.width || r >= n_rows) return;
  const int y = band_row(r, y_first, band_rows, band_pitch, n_rows);
  if (y >= S.height) return;                                               // (an entry without a pixel keeps its record)
  // the words, x0 and r0 as the first lane still here writes them; every operand is wave-uniform
  auto put = [&](uint32_t prim, bool rest, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t refl, bool flag) RT_INL {
    if (lane != (int)__builtin_ctzll(__ballot(true))) return;
    R->mask[0] = prim;
    if (!rest) return;
    const uint32_t s[4] = {s0, s1, s2, s3};
    bool lean = lean_on && prim == plane_bit && refl == 0;
    for (int l = 0; l < 4; ++l) {
      R->mask[1 + l] = s[l];
      if (l < rt_spec::N_LIGHTS) lean = lean && (s[l] & boxed) == 0;
    }
    R->mask[5] = refl;
    R->x0 = lean ? x0 | (int32_t)0x80000000u : x0;
    if (flag) R->r0 = r0 | (int32_t)0x80000000u;
  };
  V3 ro, rd;
  camera_ray_px(S, x, y, &ro, &rd);
  const DS ds = make_ds(S);
  double t_hit;
  const int oi = nearest_hit<SHARE, OBB>(ds, ro, rd, &t_hit, w[0]);
  uint32_t prim = 0;
  for (int o = 0; o < rt_spec::N_OBJECTS && o < 32; ++o)
    if (__ballot(oi == o) != 0) prim |= 1u << o;
  prim &= w[0];
  if (prim == 0) prim = keep_bit;
  const bool obj = __ballot(oi >= 0 && oi != plane) != 0;                  // a pixel on a boxed object
  if ((obj && !objects) || __ballot(oi >= 0) == 0) {                       // such an entry untraced, or sky: prim alone
    put(prim, false, 0u, 0u, 0u, 0u, 0u, false);
    return;
  }
  if (oi < 0) return;                                                      // a lane that missed takes no part in what follows
  // an object entry's words start from every object, a floor-only entry's from the predicate's
  if (obj) {
    w[1] = w[2] = w[3] = w[4] = plane_bit | boxed;
    w[5] = 0xffffffffu;
  }
  const V3 p = add(ro, scale(rd, t_hit));
  uint32_t sh[4] = {w[1], w[2], w[3], w[4]};
  _Pragma("unroll 1") for (int k = 0; k < rt_spec::N_LIGHTS && k < 4; ++k) {
    RT_REC(lt, ds, lights, LIGHTS, k);                                     // RT_HIT_LIGHTS' shadow ray: the same operations
    const V3 lv = sub(ld3(lt->p), p);
    double ll, ill;
    len_inv(lv, &ll, &ill);
    const V3 sdir = scale(lv, ill);
    const int ks = __builtin_amdgcn_readfirstlane(k);
    const uint32_t wk = ks == 0 ? w[1] : ks == 1 ? w[2] : ks == 2 ? w[3] : w[4];
    uint32_t todo = wk & boxed, occ = 0;
    // an object entry: one walk under every candidate first; no lane occluded: no one-bit walk
    if (obj && todo != 0 && __ballot(shadow_transparency<SHARE, OBB>(ds, p, sdir, ll, todo) == 0.0) == 0) todo = 0;
    _Pragma("unroll 1") while (todo != 0) {
      const uint32_t bit = (uint32_t)__builtin_amdgcn_readfirstlane((int)(todo & (0u - todo)));
      todo ^= bit;
      if (__ballot(shadow_transparency<SHARE, OBB>(ds, p, sdir, ll, bit) == 0.0) != 0) occ |= bit;
    }
    const uint32_t nw = wk & (~boxed | occ);
    if (ks == 0) sh[0] = nw; else if (ks == 1) sh[1] = nw; else if (ks == 2) sh[2] = nw; else sh[3] = nw;
  }
  V3 nrm = {0.0, 0.0, 0.0};
  Col c = {0.0, 0.0, 0.0};
  double transp = 0.0, refl = 0.0, nlen = 0.0;
  shade_inputs(ds, oi, p, &nrm, &c, &transp, &refl, &nlen);
  // trace<false> at depth 0 (max_depth > 0): a reflection where rp = refl != 0 and the hit is seen from outside
  const bool spawn = refl != 0.0 && !hit_inside(rd, nrm, nlen);
  if (__ballot(spawn) == 0) {
    put(prim, true, sh[0], sh[1], sh[2], sh[3], 0u, obj);
    return;
  }
  if (!spawn) return;
  double t1;
  const int o1 = nearest_hit<SHARE, OBB>(ds, p, reflect_dir(rd, nrm), &t1, w[5]);
  uint32_t rw = 0;
  for (int o = 0; o < rt_spec::N_OBJECTS && o < 32; ++o)
    if (__ballot(o1 == o) != 0) rw |= 1u << o;
  put(prim, true, sh[0], sh[1], sh[2], sh[3], rw & w[5], obj);
}
// The check (k_masks.hip launch_records, behind the gather and ahead of the table's `ready` event): one wave
// per entry; a candidate entry in which any valid pixel's reflected ray hits loses its bit.
// mode (wave-uniform): 0 the check; bit 0 the trace pass above in its place (one kernel: each kernel more costs
// a program 7-9 s of cold compile), bit 1 with it: the table's launches run the lean kernel, entries may say lean;
// bit 2 with it: entries with a pixel on a boxed object are traced too (`objects`).
template <bool FC>
__device__ __forceinline__ void lean_check_body(const RtDevScene& S, int y_first, int band_rows, int band_pitch, int n_rows,
                                                RtTileRec* __restrict__ recs, int mode = 0, uint32_t keep_bit = 0u) {
  if (__builtin_amdgcn_readfirstlane(mode) != 0) {
    trace_masks_body<FC>(S, y_first, band_rows, band_pitch, n_rows, recs, (mode & 2) != 0, keep_bit, (mode & 4) != 0);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int x0 = recs[blockIdx.x].x0, r0 = recs[blockIdx.x].r0;
  if (__builtin_amdgcn_readfirstlane(x0) >= 0) return;
  const int x = (x0 & 0x7fffffff) + lane % RT_TILE_W, r = r0 + lane / RT_TILE_W;
  bool hit = false;
  if (x < S.width && r < n_rows) {
    const int y = band_row(r, y_first, band_rows, band_pitch, n_rows);
    if (y < S.height) {
      V3 ro, rd;
      camera_ray_px(S, x, y, &ro, &rd);
      Col c;
      hit = lean_pixel<FC, true>(make_ds(S), ro, rd, 1, &c);
    }
  }
  if (__ballot(hit) != 0 && lane == 0) recs[blockIdx.x].x0 = x0 & 0x7fffffff;   // vector store
}
#endif

// Two-eye cameras (StereoscopicCamera / AnaglyphCamera, camera.rs:82-205; rt_blob.h RtViews): one launch
// over the tiles of two views.  Entry e (or the order's e-th) is tile e of view 0 for e < tiles0, else
// tile e - tiles0 of view 1; the wave's camera and column table are its view's (wave-uniform), the rows
// and everything past the primary ray are rows_entry's.  The walks take no tile masks.
// A view stores the channels it owns (anaglyph: the left eye R, the right eye G, B and A -- disjoint bytes
// of one pixel, so the two eyes' waves need no order and every output byte is written once): RGBA8 as a
// byte, or a byte and an aligned 16-bit B | 255 << 8; RGB8 as bytes; f64 as o[0] or o[1..3].
template <bool F64>
__device__ __forceinline__ void store_pixel_view(uint8_t* row, int x, Col c, int rgb, int channels) {
  if (channels == RT_VIEW_RGBA) {
    store_pixel<F64>(row, x, c, rgb);
  } else if constexpr (F64) {
    double* o = (double*)row + (size_t)x * 4;
    if (channels == RT_VIEW_R) o[0] = c.r;
    else { o[1] = c.g; o[2] = c.b; o[3] = 1.0; }
  } else if (rgb) {
    uint8_t* o = row + (size_t)x * 3;
    if (channels == RT_VIEW_R) frame_store((uint8_t)to_u8(c.r), o);
    else { frame_store((uint8_t)to_u8(c.g), o + 1); frame_store((uint8_t)to_u8(c.b), o + 2); }
  } else {
    uint8_t* o = row + (size_t)x * 4;
    if (channels == RT_VIEW_R) frame_store((uint8_t)to_u8(c.r), o);
    else { frame_store((uint8_t)to_u8(c.g), o + 1); frame_store((unsigned short)(to_u8(c.b) | (255u << 8)), (unsigned short*)(o + 2)); }
  }
}
template <int MODE, bool F64, bool CAL, bool FC, int KL_ = -1, int KP_ = -1>
__device__ __forceinline__ void rows_views_body(const RtDevScene& S, const RtViews& VW, int y_first, int band_rows,
                                                int band_pitch, int n_rows, int max_depth, uint8_t* __restrict__ out,
                                                size_t stride, const int32_t* __restrict__ order,
                                                uint32_t* __restrict__ cost, int rgb, lds_f64* frames) {
  constexpr bool REFR = MODE != RT_MODE_REFL, CHAIN = MODE == RT_MODE_CHAIN;
  constexpr int KLR = MODE == RT_MODE_TREE ? RT_LDS_RFRAMES : 0;
  constexpr int KP = rows_pool_slots<MODE, KL_, KP_>();
  constexpr int KL = rows_lane_frames<MODE, KL_>();
  const int lane = threadIdx.x & 63;
  const unsigned entry = CAL || !order ? blockIdx.x : (unsigned)order[blockIdx.x];
  [[maybe_unused]] uint64_t t_start = 0;
  if constexpr (CAL) t_start = wall_clock64();
  const int vi = __builtin_amdgcn_readfirstlane(entry >= (unsigned)VW.tiles0 ? 1 : 0);
  const RtView& V = VW.v[vi];
  const unsigned tile = entry - (vi ? (unsigned)VW.tiles0 : 0u);
  const int xv = (int)(tile % (unsigned)V.tiles_x) * RT_TILE_W + lane % RT_TILE_W;   // the view's own column
  const int r = (int)(tile / (unsigned)V.tiles_x) * RT_TILE_H + lane / RT_TILE_W;
  if (xv >= V.width || r >= n_rows) return;
  const int y = band_row(r, y_first, band_rows, band_pitch, n_rows);
  if (y >= S.height) return;
  const double sx = V.cam_sx[xv], sy = S.cam_sy[y];                          // create_ray(xv as f64, y as f64)
  const V3 rd = add(add(ld3(V.cam.direction), scale(ld3(V.cam.right), sx)), scale(ld3(V.cam.up), sy));
  const V3 ro = ld3(V.cam.center);
  const Col c = trace<REFR, NoRec, KL, FC, KLR, CHAIN, KP>(make_ds(S), ro, rd, max_depth, nullptr, frames + lane, frames);
  store_pixel_view<F64>(out + (size_t)r * stride, V.x0 + xv, c, rgb, V.channels);
  if constexpr (CAL)
    if (threadIdx.x == 0) cost[entry] = (uint32_t)(wall_clock64() - t_start);   // vector store
}
template <int MODE, int KL_ = -1, int KP_ = -1>
constexpr int rows_lds_doubles() {
  return (rows_lane_frames<MODE, KL_>() * 4 + (MODE == RT_MODE_TREE ? RT_LDS_RFRAMES : 0) * 7) * 64 +
         (rows_pool_slots<MODE, KL_, KP_>() > 0
              ? RT_POOL_HDR + pool_doubles<rows_pool_slots<MODE, KL_, KP_>(), RT_POOL_OBJ_INDEX != 0>()
              : 0);
}

// The sample kernels' bodies (the specialised programs rt_spec_points / rt_spec_aa, spec_text.cpp): get_pixel at
// any (x, y) for rt_render_points_f64 and for the anti-aliasing pass's requested sub-pixels, with the frame
// storage of the scene's mode exactly as rows_entry takes it for a non-PRIM launch (frames: the one-wave
// workgroup's s_frames of rows_lds_doubles<MODE, KL_, KP_>() doubles).  No tile masks: a sample is in no tile.
// Lane i of the launch traces sample i; lanes past n leave before trace(), as in the generic kernels
// (k_points.hip render_points_kernel, k_aa.hip aa_trace_kernel), whose stores these repeat.
template <int MODE, bool FC, int KL_ = -1, int KP_ = -1>
__device__ __forceinline__ void points_body(const RtDevScene& S, const double* __restrict__ xy, size_t n, int max_depth,
                                            double* __restrict__ out, lds_f64* frames) {
  constexpr bool REFR = MODE != RT_MODE_REFL, CHAIN = MODE == RT_MODE_CHAIN;
  constexpr int KLR = MODE == RT_MODE_TREE ? RT_LDS_RFRAMES : 0;
  constexpr int KP = rows_pool_slots<MODE, KL_, KP_>();
  constexpr int KL = rows_lane_frames<MODE, KL_>();
  const int lane = threadIdx.x & 63;
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  V3 ro, rd;
  camera_ray(S.cam, xy[2 * i], xy[2 * i + 1], &ro, &rd);
  const Col c = trace<REFR, NoRec, KL, FC, KLR, CHAIN, KP>(make_ds(S), ro, rd, max_depth, nullptr, frames + lane, frames);
  out[4 * i] = c.r; out[4 * i + 1] = c.g; out[4 * i + 2] = c.b; out[4 * i + 3] = 1.0;
}
// Request i of an anti-aliasing pass: req[2 * i] = the edge pixel's index e, req[2 * i + 1] = sx | sy << 8;
// edges[e] = x | y << 16; the colour goes to grid point [sx][sy] of pixel e's size x size grid in col
// (4 doubles per point).  The sample position's operations are the reference's (antialiaser.rs:108-112).
template <int MODE, bool FC, int KL_ = -1, int KP_ = -1>
__device__ __forceinline__ void aa_trace_body(const RtDevScene& S, const uint32_t* __restrict__ edges,
                                              const uint32_t* __restrict__ req, uint32_t n, int size,
                                              double* __restrict__ col, int max_depth, lds_f64* frames) {
  constexpr bool REFR = MODE != RT_MODE_REFL, CHAIN = MODE == RT_MODE_CHAIN;
  constexpr int KLR = MODE == RT_MODE_TREE ? RT_LDS_RFRAMES : 0;
  constexpr int KP = rows_pool_slots<MODE, KL_, KP_>();
  constexpr int KL = rows_lane_frames<MODE, KL_>();
  const int lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = req[2 * (size_t)i], s = req[2 * (size_t)i + 1];
  const int x = edges[e] & 0xffff, y = edges[e] >> 16;
  const int sx = s & 0xff, sy = s >> 8;
  V3 ro, rd;
  camera_ray(S.cam, (double)x + ((double)sx / (double)size), (double)y + ((double)sy / (double)size), &ro, &rd);
  const Col c = trace<REFR, NoRec, KL, FC, KLR, CHAIN, KP>(make_ds(S), ro, rd, max_depth, nullptr, frames + lane, frames);
  double* o = col + ((size_t)e * size * size + sx * size + sy) * 4;
  o[0] = c.r; o[1] = c.g; o[2] = c.b; o[3] = 1.0;
}

// The deferred-shadow kernel's body (reflection-only scenes, or refraction chains on request): one
// wave per 8x8 tile, every tile on the deferred path (trace_deferred), and the costliest tiles split
// over P = 2, 4 or 8 waves: wave `part` renders pixels [part * 64/P, (part + 1) * 64/P) of the tile
// on its first 64/P lanes and its other lanes only trace shadow rays (phase 2).  Order entry:
// tile | part << 20 | log2(P) << 24 (built by launch_bands after the calibration launch).
#define RT_SPLIT_TILE_MASK 0xFFFFFu   // order entries: tile index in bits 0-19
static_assert(RT_SPLIT_MAX_LOG2 <= 4, "split part index has 4 bits");
template <bool F64, bool CAL, bool FC, bool REFR>
__device__ __forceinline__ void deferred_body(const RtDevScene& S, int y_first, int band_rows, int band_pitch,
                                              int n_rows, int max_depth, uint8_t* __restrict__ out, size_t stride,
                                              const int32_t* __restrict__ order, uint32_t* __restrict__ cost, int rgb,
                                              ShadowWin* win) {
  const int lane = threadIdx.x & 63;
  const uint32_t e = CAL || !order ? blockIdx.x : (uint32_t)order[blockIdx.x];
  const unsigned tile = e & RT_SPLIT_TILE_MASK;
  const int lp = (int)((e >> 24) & 7u), per = 64 >> lp;
  const int pix = (int)((e >> 20) & 15u) * per + lane;
  [[maybe_unused]] uint64_t t_start = 0;
  if constexpr (CAL) t_start = wall_clock64();
  int x, r;
  tile_pixel(tile, pix, S.width, &x, &r);
  int y = 0;
  bool valid = lane < per && x < S.width && r < n_rows;
  if (valid) {
    y = band_row(r, y_first, band_rows, band_pitch, n_rows);
    valid = y < S.height;
  }
  V3 ro = {0.0, 0.0, 0.0}, rd = {0.0, 0.0, 0.0};
  if (valid) camera_ray_px(S, x, y, &ro, &rd);                              // get_pixel(x as f64, y as f64)
  const Col c = trace_deferred<RT_MAX_DEPTH_CAP + 1, FC, REFR>(make_ds(S), ro, rd, max_depth, valid, win);
  if (valid) store_pixel<F64>(out + (size_t)r * stride, x, c, rgb);
  if constexpr (CAL)
    if (lane == 0) cost[tile] = (uint32_t)(wall_clock64() - t_start);
}

}  // namespace
