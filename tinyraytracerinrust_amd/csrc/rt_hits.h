// rt_hits.h -- a sample's FIRST HIT without its shading (k_hits.hip; after rt_device.h): the object a camera ray
// hits first, the distance, which lights' shadow rays are occluded at the hit point and the shape's raw normal
// there -- get_ray_color's steps up to the light loop (raytracer.rs:141-150, :162, :176-197) and the ray
// debugger's get_normal (ray_debugger.rs:113-119), through the walks every render kernel takes (rt_walks.h).
#pragma once

namespace {

struct FirstHit {
  int object;          // draw index, -1 = miss
  double distance;     // INFINITY on a miss
  uint32_t shadow;     // bit k: light k's shadow ray is occluded (transparency != 1.0)
  V3 normal;           // the shape's get_normal at the hit point, not normalised; zeros on a miss
};

// REFR chooses the walks as trace() does for the scene's mode (rt_trace.h: SHARE = REFR, OBB = !REFR), so the hit
// and the shadow products are the render kernels' own.  SHADOW / NORMAL: whether the shadow bits and the normal
// are produced at all; an instantiation without them holds no shadow walk and no normal code.
template <bool REFR, bool SHADOW, bool NORMAL>
RT_FN FirstHit first_hit(const DS& S, V3 ro, V3 rd) {
  constexpr bool SHARE = REFR, OBB = !REFR;
  FirstHit h = {-1, INFINITY, 0u, {0.0, 0.0, 0.0}};
  double t;
  const int oi = nearest_hit<SHARE, OBB>(S, ro, rd, &t);                  // :141-150
  if (oi < 0) return h;
  h.object = oi;
  h.distance = t;
  const V3 p = add(ro, scale(rd, t));                                      // :162
  if constexpr (SHADOW) {
#pragma unroll 1
    for (int k = 0; k < S.n_lights; ++k) {                                 // sdir, ll as RT_HIT_LIGHTS forms them
      RT_REC(lt, S, lights, LIGHTS, k);
      const V3 lv = sub(ld3(lt->p), p);
      double ll, ill;
      len_inv(lv, &ll, &ill);
      const V3 sdir = scale(lv, ill);
      if (shadow_transparency<SHARE, OBB>(S, p, sdir, ll) != 1.0) h.shadow |= 1u << k;   // :176-197
    }
  }
  if constexpr (NORMAL) {
    // scalarised over the distinct objects hit in the wave, as shade_inputs: object_normal_uv reads the object's
    // records wave-uniformly and votes (ballots) among the lanes it is called for
    uint64_t todo = __ballot(true);
    while (todo) {
      const int o = __builtin_amdgcn_readlane(oi, (int)__builtin_ctzll(todo));
      const uint64_t mine = __ballot(oi == o);
      todo &= ~mine;
      if ((mine >> __lane_id()) & 1) {
        double u, v;
        object_normal_uv(S, &S.objects[o], p, false, &h.normal, &u, &v);    // ray_debugger.rs:113-119
      }
    }
  }
  return h;
}

}  // namespace
