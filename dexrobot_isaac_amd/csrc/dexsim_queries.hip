// dexsim_queries.hip -- libdexsim's query unit: the C-ABI (include/dexsim.h) of the queries on a simulation's state -- camera
// sensors, Jacobians and mass matrix, inverse kinematics, clearances, range sensors, inverse dynamics, forward kinematics, forward
// dynamics and the dynamics derivatives -- over their gfx950 kernels (dexsim_chain, _render, _kindyn, _ik, _proximity, _raycast, _invdyn,
// _fk, _fwddyn, _dynderiv).
//
// The library's second translation unit (build: see dexsim.hip).  It includes none of the step unit's .hip.inc files and the step
// unit none of these; from the step side it takes the declarations of dexsim_device.h and the handle of dexsim_host.h, nothing
// flows back.  Each family's kernels are included in front of their entry points, a later family behind the ones it builds on.
#include <cmath>
#include <algorithm>
#include "dexsim_host.h"

#include <cstdio>
#include <cstring>
#include <string>

// ------------------------------------------------------------------------------------------------- camera sensors
// clang-format off
#include "dexsim_chain.hip.inc"
#include "dexsim_render.hip.inc"
// clang-format on

extern "C" int dexsim_camera_struct_size(size_t* out) {
  if (!out) return fail(DEXSIM_ERR_ARG, "dexsim_camera_struct_size: null argument");
  *out = sizeof(DexSimCamera);
  return DEXSIM_OK;
}

extern "C" int dexsim_render_layout(DexSimField* fields, int max_fields, int* n_fields, size_t* scene_words) {
  if (!n_fields || !scene_words) return fail(DEXSIM_ERR_ARG, "dexsim_render_layout: bad argument");
  int n = 0, end = 0;
  for (const RenderSection& s : kRenderSections) {
    if (fields) {
      if (n >= max_fields) return fail(DEXSIM_ERR_LAYOUT, "field table too small");
      std::snprintf(fields[n].name, sizeof fields[n].name, "%s", s.name);
      fields[n].rows = s.words; fields[n].is_int = s.is_int; fields[n].offset = (size_t)s.off;
    }
    end = s.off + s.words;
    n++;
  }
  *n_fields = n;
  *scene_words = (size_t)end;
  return DEXSIM_OK;
}

extern "C" int dexsim_render(dexsim_t h, const DexSimCamera* cam, const float* eye, const float* target, const int64_t* env_ids, int k,
                             float* scene, float* depth, uint8_t* rgba, int32_t* seg, void* stream) {
  if (!h || !h->bound) return fail(DEXSIM_ERR_ARG, "dexsim_render: null or unbound handle");
  if (!cam || !scene) return fail(DEXSIM_ERR_ARG, "dexsim_render: camera and scene workspace are required");
  if (!depth && !rgba && !seg) return fail(DEXSIM_ERR_ARG, "dexsim_render: at least one of depth, rgba and seg is required");
  if (((uintptr_t)scene & 15) != 0 || ((uintptr_t)rgba & 3) != 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_render: the scene workspace must be 16-byte aligned, rgba 4-byte aligned");
  if (cam->width < 1 || cam->width > DEXSIM_RENDER_MAX_DIM || cam->height < 1 || cam->height > DEXSIM_RENDER_MAX_DIM)
    return fail(DEXSIM_ERR_ARG, "dexsim_render: width and height must be in [1, 4096]");
  if (!(cam->hfov_deg > 0.f && cam->hfov_deg < 180.f)) return fail(DEXSIM_ERR_ARG, "dexsim_render: hfov_deg must be in (0, 180)");
  if (!(cam->near_clip < cam->far_clip)) return fail(DEXSIM_ERR_ARG, "dexsim_render: near_clip must be below far_clip");
  if (cam->parent_joint < -1 || cam->parent_joint >= DEXSIM_NJ) return fail(DEXSIM_ERR_ARG, "dexsim_render: parent_joint out of range");
  if (!env_ids) k = h->N;
  if (k < 0) return fail(DEXSIM_ERR_ARG, "dexsim_render: k must not be negative");
  const long long npix = (long long)cam->width * cam->height;
  if ((long long)k * npix >= (1ll << 31)) return fail(DEXSIM_ERR_ARG, "dexsim_render: k * width * height must stay below 2^31");
  if (k == 0) return DEXSIM_OK;
  DeviceGuard guard(h->device);
  RenderArgs R;
  R.cam = *cam; R.eye = eye; R.target = target; R.env_ids = env_ids; R.k = k; R.img0 = 0;
  const double t = std::tan(0.5 * (double)cam->hfov_deg * 3.14159265358979323846 / 180.0);
  R.tan_x = (float)t; R.tan_y = (float)(t * (double)cam->height / (double)cam->width);
  auto* ks = cam->parent_joint >= 0 ? k_render_scene<true> : k_render_scene<false>;
  auto* kr = h->cfg.has_box ? k_render_rays<true> : k_render_rays<false>;
  ks<<<dim3((k + 63) / 64), dim3(64), 0, (hipStream_t)stream>>>(h->d_params, R, scene, h->NS, h->N);
  LAUNCH_CHECK();
  const RayOut O{depth, (unsigned*)rgba, (int*)seg};
  const int ymax = 32768;   // images per launch (extent of the grid's y dimension)
  for (int i0 = 0; i0 < k; i0 += ymax) {
    R.img0 = i0;
    kr<<<dim3((unsigned)((npix + 255) / 256), (unsigned)std::min(ymax, k - i0)), dim3(256), 0, (hipStream_t)stream>>>(scene, R, O, h->N);
    LAUNCH_CHECK();
  }
  return DEXSIM_OK;
}

// ------------------------------------------------------------------------------------------------- Jacobians, mass matrix, gravity force
// clang-format off
#include "dexsim_kindyn.hip.inc"
// clang-format on

// The checks both entry points share; none of them needs a device.  k is the number of output rows.
static int kin_rows(const char* who, dexsim_t h, const int64_t* env_ids, int k, const float* q, KinRows* R) {
  if (!h) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": null handle").c_str());
  if (k <= 0) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": k must be positive").c_str());
  if (!q && !env_ids && k != h->N) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": env_ids == NULL without a q override needs k == num_envs").c_str());
  R->env_ids = q ? nullptr : env_ids; R->q = q; R->k = k;
  return DEXSIM_OK;
}

// The box of a geometric query (KinBox, dexsim_chain.hip.inc): the caller's (k, 7) box_pose, else the env's own box on the state path
// of a task that has one, else none; box_size > 0 overrides cfg.box_size.  Behind kin_rows (it reads the handle); that box_size is
// finite needs no handle and is checked by the entry points in front of it.
static int kin_box(const char* who, dexsim_t h, const float* q, const float* box_pose, float box_size, KinBox* B) {
  const float size = box_size > 0.f ? box_size : h->cfg.box_size;
  B->pose = box_pose;
  B->env = !box_pose && !q && h->cfg.has_box;
  if ((B->pose || B->env) && !(size > 0.f)) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": a box needs a positive box_size or cfg.box_size").c_str());
  B->hb = 0.5f * size;
  return DEXSIM_OK;
}

// a required output: non-NULL and `align`-byte aligned
static int kin_out(const char* who, const char* name, const void* p, int align) {
  if (p && ((uintptr_t)p & (uintptr_t)(align - 1)) == 0) return DEXSIM_OK;
  return fail(DEXSIM_ERR_ARG, (std::string(who) + ": " + name + " must be a " + std::to_string(align) + "-byte aligned device pointer").c_str());
}

// A request of nb hand bodies (NULL = all of them, in order): the checks of the list, then of the output `name`, then that the
// model's bodies ride on the frames kd_body_joint says.  body[i], where given, receives the i-th requested body.
static int kin_bodies(const char* who, dexsim_t h, const int* bodies, int nb, unsigned char* body, const char* name, const void* out, int align) {
  const std::string w(who);
  if (nb < 1 || nb > DEXSIM_NUM_HAND_BODIES) return fail(DEXSIM_ERR_ARG, (w + ": nb must be in [1, DEXSIM_NUM_HAND_BODIES]").c_str());
  if (!bodies && nb != DEXSIM_NUM_HAND_BODIES) return fail(DEXSIM_ERR_ARG, (w + ": bodies == NULL needs nb == DEXSIM_NUM_HAND_BODIES").c_str());
  for (int i = 0; i < nb; i++) {
    const int b = bodies ? bodies[i] : i;
    if (b < 0 || b >= DEXSIM_NUM_HAND_BODIES) return fail(DEXSIM_ERR_ARG, (w + ": body index out of range").c_str());
    if (body) body[i] = (unsigned char)b;
  }
  int rc = kin_out(who, name, out, align);
  if (rc) return rc;
  for (int b = 0; b < DEXSIM_NUM_HAND_BODIES; b++)
    if (h->model.body_parent[b] != kd_body_joint(b))
      return fail(DEXSIM_ERR_ARG, (w + ": model.body_parent differs from the frames rigid_body_states is published on").c_str());
  return DEXSIM_OK;
}

// the family's grid: 64 rows per workgroup of KD_THREADS, `gy` workgroups along y
#define KIN_LAUNCH(kernel, gy, args)                                                                                              \
  kernel<<<dim3((unsigned)((k + 63) / 64), (unsigned)(gy)), dim3(KD_THREADS), 0, (hipStream_t)stream>>>(h->d_params, args, h->NS, h->N); \
  LAUNCH_CHECK()

extern "C" int dexsim_body_jacobian(dexsim_t h, const int64_t* env_ids, int k, const float* q, const int* bodies, int nb, float* jac,
                                    void* stream) {
  KinJac J;
  std::memset(&J, 0, sizeof J);
  int rc = kin_rows("dexsim_body_jacobian", h, env_ids, k, q, &J.rows);
  if (rc) return rc;
  rc = kin_bodies("dexsim_body_jacobian", h, bodies, nb, J.body, "jac", jac, 16);
  if (rc) return rc;
  NEED_BOUND(h);
  J.jac = jac; J.nb = nb;
  KIN_LAUNCH(k_kin_jacobian, (nb + KJ_CHUNK - 1) / KJ_CHUNK, J);
  return DEXSIM_OK;
}

extern "C" int dexsim_mass_matrix(dexsim_t h, const int64_t* env_ids, int k, const float* q, float* mass, float* gravity, void* stream) {
  KinMass K;
  std::memset(&K, 0, sizeof K);
  int rc = kin_rows("dexsim_mass_matrix", h, env_ids, k, q, &K.rows);
  if (rc) return rc;
  if (!mass && !gravity) return fail(DEXSIM_ERR_ARG, "dexsim_mass_matrix: at least one of mass and gravity is required");
  if (((uintptr_t)mass & 15) != 0 || ((uintptr_t)gravity & 3) != 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_mass_matrix: mass must be 16-byte aligned, gravity 4-byte aligned");
  NEED_BOUND(h);
  K.mass = mass; K.gravity = gravity;
  KIN_LAUNCH(k_kin_mass, 1, K);
  return DEXSIM_OK;
}

// ------------------------------------------------------------------------------------------------- fingertip inverse kinematics
// clang-format off
#include "dexsim_ik.hip.inc"
// clang-format on

extern "C" int dexsim_ik_struct_size(size_t* out) {
  if (!out) return fail(DEXSIM_ERR_ARG, "dexsim_ik_struct_size: null argument");
  *out = sizeof(DexSimIK);
  return DEXSIM_OK;
}

extern "C" int dexsim_solve_ik(dexsim_t h, const int64_t* env_ids, int k, const float* q0, const float* targets, const DexSimIK* prm,
                               float* controls, float* q_out, float* residual, void* stream) {
  // the parameter checks need neither a handle nor a device
  if (!targets || !controls || !prm) return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: targets, controls and prm are required");
  if (prm->sites < 0 || prm->sites > 1) return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: sites must be 0 (fingertips) or 1 (fingerpads)");
  if (prm->frame < 0 || prm->frame > 1) return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: frame must be 0 (world) or 1 (hand)");
  if (prm->free_mask == 0 || (prm->free_mask >> DEXSIM_NACT) != 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: free_mask must have at least one of its bits 0..17 set and none above");
  if (prm->frame == 1 && (prm->free_mask & 63u) != 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: hand-frame targets (frame 1) need the base controls 0..5 fixed");
  if (prm->iters < 1 || prm->iters > DEXSIM_IK_MAX_ITERS) return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: iters must be in [1, DEXSIM_IK_MAX_ITERS]");
  if (!(prm->damping > 0.f) || !std::isfinite(prm->damping)) return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: damping must be positive");
  if (!(prm->max_step > 0.f) || !std::isfinite(prm->max_step)) return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: max_step must be positive");
  float wsum = 0.f;
  for (int f = 0; f < DEXSIM_NFINGER; f++) {
    if (!(prm->weight[f] >= 0.f) || !std::isfinite(prm->weight[f])) return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: a weight is negative");
    wsum += prm->weight[f];
  }
  if (!(wsum > 0.f)) return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: the weights are all zero");
  if (k <= 0) return fail(DEXSIM_ERR_ARG, "dexsim_solve_ik: k must be positive");
  IkArgs K;
  std::memset(&K, 0, sizeof K);
  int rc = kin_rows("dexsim_solve_ik", h, env_ids, k, q0, &K.rows);
  if (rc) return rc;
  NEED_BOUND(h);
  K.targets = targets; K.controls = controls; K.q_out = q_out; K.residual = residual;
  K.prm = *prm; K.lam2 = prm->damping * prm->damping;
  KIN_LAUNCH(k_ik_solve, 1, K);
  return DEXSIM_OK;
}

// ------------------------------------------------------------------------------------------------- clearance queries
// clang-format off
#include "dexsim_proximity.hip.inc"
// clang-format on

// pair i of the pair table (include/dexsim.h), in the capsule order validate_model and dexsim_query_proximity insist on
static void px_pair(int i, int* cap_a, int* cap_b, int* group) {
  if (i < 90) {
    const int g = i / 9, r = i - 9 * g;
    *cap_a = kd_finger_cap(px_group_fa(g), r / 3); *cap_b = kd_finger_cap(px_group_fb(g), r % 3); *group = g;
  } else {
    const int j = i - 90, f = j / 6, r = j - 6 * f;
    *cap_a = r / 2; *cap_b = kd_finger_cap(f, 1 + r % 2); *group = 10 + f;
  }
}

extern "C" int dexsim_proximity_pair(int i, int* cap_a, int* cap_b, int* group) {
  if (!cap_a || !cap_b || !group) return fail(DEXSIM_ERR_ARG, "dexsim_proximity_pair: null argument");
  if (i < 0 || i >= DEXSIM_NPROX_PAIRS) return fail(DEXSIM_ERR_ARG, "dexsim_proximity_pair: pair index out of range");
  px_pair(i, cap_a, cap_b, group);
  return DEXSIM_OK;
}

extern "C" int dexsim_query_proximity(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* box_pose, float box_size,
                                      float* cap_env, float* self_min, float* pair_dist, void* stream) {
  // the checks of the outputs, of box_size and of k need neither a handle nor a device
  if (!cap_env && !self_min && !pair_dist)
    return fail(DEXSIM_ERR_ARG, "dexsim_query_proximity: at least one of cap_env, self_min and pair_dist is required");
  if (((uintptr_t)cap_env & 15) != 0 || ((uintptr_t)self_min & 15) != 0 || ((uintptr_t)pair_dist & 15) != 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_query_proximity: the outputs must be 16-byte aligned");
  if (!std::isfinite(box_size)) return fail(DEXSIM_ERR_ARG, "dexsim_query_proximity: box_size is not finite");
  if (k <= 0) return fail(DEXSIM_ERR_ARG, "dexsim_query_proximity: k must be positive");
  ProxArgs K;
  std::memset(&K, 0, sizeof K);
  int rc = kin_rows("dexsim_query_proximity", h, env_ids, k, q, &K.rows);
  if (rc) return rc;
  for (int c = 0; c < DEXSIM_NCAP; c++)
    if (h->model.cap_fslot[c] != (c < 3 ? DEXSIM_FSLOT_PALM : c - 3))
      return fail(DEXSIM_ERR_ARG, "dexsim_query_proximity: the model must have exactly three palm capsules (0-2) and one capsule per finger "
                                  "link (capsule 3 + s in force slot s)");
  rc = kin_box("dexsim_query_proximity", h, q, box_pose, box_size, &K.box);
  if (rc) return rc;
  NEED_BOUND(h);
  K.cap_env = cap_env; K.self_min = self_min; K.pair_dist = pair_dist;
  KIN_LAUNCH(k_proximity, 1, K);
  return DEXSIM_OK;
}

// ------------------------------------------------------------------------------------------------- range sensors
// The rows and the box of a call as for the clearances: kin_rows, kin_box.
// clang-format off
#include "dexsim_raycast.hip.inc"
// clang-format on

extern "C" int dexsim_raycast(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* box_pose, float box_size,
                              const float* rays, const int* parent, int nrays, float min_range, float max_range, int flags,
                              float* dist, float* hits, void* stream) {
  // the checks of the ray list, the window, the flags, the outputs, of box_size and of k need neither a handle nor a device
  if (nrays < 1 || nrays > DEXSIM_RAY_MAX) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: nrays must be in [1, DEXSIM_RAY_MAX]");
  if (!rays || !parent) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: rays and parent are required");
  RayArgs K;
  std::memset(&K, 0, sizeof K);
  for (int i = 0, j = -1; i <= nrays; i++) {   // the prefix offsets of the parent groups
    const int p = i < nrays ? parent[i] : DEXSIM_NJ;
    if (i < nrays && (p < -1 || p >= DEXSIM_NJ)) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: a parent is outside [-1, DEXSIM_NJ)");
    if (p < j) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: parent must be non-decreasing (sort the rays by parent)");
    if (i == 0) K.jstart[0] = 0;
    for (; j < p; j++) K.jstart[j + 2] = (unsigned short)i;   // group j ends, group j + 1 begins at ray i
  }
  if (!std::isfinite(min_range) || !std::isfinite(max_range) || min_range < 0.f || !(min_range < max_range))
    return fail(DEXSIM_ERR_ARG, "dexsim_raycast: the ranges must be finite with 0 <= min_range < max_range");
  if ((flags & ~DEXSIM_RAY_SKIP_PARENT) != 0) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: unknown flag bits (DEXSIM_RAY_SKIP_PARENT is the only flag)");
  if (!dist && !hits) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: at least one of dist and hits is required");
  if (((uintptr_t)dist & 15) != 0 || ((uintptr_t)hits & 15) != 0) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: the outputs must be 16-byte aligned");
  if (!std::isfinite(box_size)) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: box_size is not finite");
  if (k <= 0) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: k must be positive");
  int rc = kin_rows("dexsim_raycast", h, env_ids, k, q, &K.rows);
  if (rc) return rc;
  if (flags & DEXSIM_RAY_SKIP_PARENT)
    for (int c = 0; c < DEXSIM_NCAP; c++) {
      const int p = h->model.cap_parent[c];
      if (p < 0 || p >= DEXSIM_NJ) return fail(DEXSIM_ERR_ARG, "dexsim_raycast: DEXSIM_RAY_SKIP_PARENT needs every model.cap_parent in [0, DEXSIM_NJ)");
      K.skip[p] |= 1u << c;
    }
  rc = kin_box("dexsim_raycast", h, q, box_pose, box_size, &K.box);
  if (rc) return rc;
  NEED_BOUND(h);
  K.rays = rays; K.nrays = nrays;
  K.tmin = min_range; K.tmax = max_range;
  K.dist = dist; K.hits = hits;
  KIN_LAUNCH(k_raycast, (nrays + RC_CHUNK - 1) / RC_CHUNK, K);
  return DEXSIM_OK;
}

// ------------------------------------------------------------------------------------------------- inverse dynamics, bias accelerations
// clang-format off
#include "dexsim_invdyn.hip.inc"
// clang-format on

// kin_rows plus the rule of the velocity override: q and qd are both NULL (arena) or both (k, 26) overrides
static int kin_rows_qd(const char* who, dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd, KinRows* R) {
  int rc = kin_rows(who, h, env_ids, k, q, R);
  if (rc) return rc;
  if (!q != !qd) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": q and qd must both be NULL (the envs' state) or both be (k, 26) overrides").c_str());
  return DEXSIM_OK;
}

// The `n` requested bodies bodies[first + i] (NULL: body first + i) sorted by the frame they ride on -- -1 (the spawn frame), then
// the joints in order -- from entry `at` on: body[] and slot[] (i, the position in the request) per entry, one range per frame in
// jstart[0 .. DEXSIM_NJ + 1], so that a wave visits its own bodies only.  Returns the end of the entries.
static int kin_sort_by_frame(const int* bodies, int first, int n, int at, unsigned char* body, unsigned char* slot, unsigned char* jstart) {
  for (int j = -1; j < DEXSIM_NJ; j++) {
    jstart[j + 1] = (unsigned char)at;
    for (int i = 0; i < n; i++) {
      const int b = bodies ? bodies[first + i] : first + i;
      if (kd_body_joint(b) == j) { body[at] = (unsigned char)b; slot[at] = (unsigned char)i; at++; }
    }
  }
  jstart[DEXSIM_NJ + 1] = (unsigned char)at;
  return at;
}

extern "C" int dexsim_inverse_dynamics(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd, const float* qdd,
                                       int flags, float* tau, void* stream) {
  InvDyn K;
  std::memset(&K, 0, sizeof K);
  int rc = kin_rows_qd("dexsim_inverse_dynamics", h, env_ids, k, q, qd, &K.rows);
  if (rc) return rc;
  if ((flags & ~DEXSIM_ID_GRAVITY) != 0) return fail(DEXSIM_ERR_ARG, "dexsim_inverse_dynamics: unknown flag bits (DEXSIM_ID_GRAVITY is the only flag)");
  if ((rc = kin_out("dexsim_inverse_dynamics", "tau", tau, 4))) return rc;
  NEED_BOUND(h);
  K.qd = qd; K.qdd = qdd; K.tau = tau; K.gravity = flags & DEXSIM_ID_GRAVITY;
  KIN_LAUNCH(k_kin_invdyn, 1, K);
  return DEXSIM_OK;
}

extern "C" int dexsim_body_bias_accel(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd, const int* bodies, int nb,
                                      float* acc, void* stream) {
  BiasAcc K;
  std::memset(&K, 0, sizeof K);
  int rc = kin_rows_qd("dexsim_body_bias_accel", h, env_ids, k, q, qd, &K.rows);
  if (rc) return rc;
  rc = kin_bodies("dexsim_body_bias_accel", h, bodies, nb, nullptr, "acc", acc, 4);
  if (rc) return rc;
  kin_sort_by_frame(bodies, 0, nb, 0, K.body, K.slot, K.jstart);
  NEED_BOUND(h);
  K.qd = qd; K.acc = acc; K.nb = nb;
  KIN_LAUNCH(k_kin_bias_accel, 1, K);
  return DEXSIM_OK;
}

// ------------------------------------------------------------------------------------------------- forward kinematics
// Behind the inverse dynamics: the kernel uses its velocity walk.
// clang-format off
#include "dexsim_fk.hip.inc"
// clang-format on

extern "C" int dexsim_forward_kinematics(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd, const int* bodies,
                                         int nb, int flags, float* body_states, float* site_poses, float* centroid, void* stream) {
  FwdKin K;
  std::memset(&K, 0, sizeof K);
  int rc = kin_rows("dexsim_forward_kinematics", h, env_ids, k, q, &K.rows);
  if (rc) return rc;
  if (qd && !q) return fail(DEXSIM_ERR_ARG, "dexsim_forward_kinematics: a qd override needs a q override (the state path takes the envs' qd)");
  if ((flags & ~DEXSIM_FK_HAND_FRAME) != 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_forward_kinematics: unknown flag bits (DEXSIM_FK_HAND_FRAME is the only flag)");
  if (!body_states && !site_poses && !centroid)
    return fail(DEXSIM_ERR_ARG, "dexsim_forward_kinematics: at least one of body_states, site_poses and centroid is required");
  if (body_states && (rc = kin_bodies("dexsim_forward_kinematics", h, bodies, nb, nullptr, "body_states", body_states, 4))) return rc;
  if (((uintptr_t)site_poses & 3) != 0 || ((uintptr_t)centroid & 15) != 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_forward_kinematics: site_poses must be 4-byte aligned, centroid 16-byte aligned");
  NEED_BOUND(h);
  K.qd = qd; K.body_states = body_states; K.site_poses = site_poses; K.centroid = centroid;
  K.nb = body_states ? nb : 0; K.nby = (K.nb + FK_CHUNK - 1) / FK_CHUNK;
  K.vel = !q || qd; K.hand_frame = flags & DEXSIM_FK_HAND_FRAME;
  for (int c = 0, at = 0; c < K.nby; c++)   // every chunk of the request sorted on its own
    at = kin_sort_by_frame(bodies, c * FK_CHUNK, std::min(FK_CHUNK, K.nb - c * FK_CHUNK), at, K.body, K.slot, K.jstart[c]);
  KIN_LAUNCH(k_kin_fk, K.nby + (site_poses || centroid ? 1 : 0), K);
  return DEXSIM_OK;
}

// ------------------------------------------------------------------------------------------------- forward dynamics, mass-matrix solves
// Behind the inverse dynamics: the kernel uses its Newton-Euler helpers.
// clang-format off
#include "dexsim_fwddyn.hip.inc"
// clang-format on

extern "C" int dexsim_forward_dynamics(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd, const float* tau,
                                       int flags, float* qdd, void* stream) {
  FwdDyn K;
  std::memset(&K, 0, sizeof K);
  int rc = kin_rows_qd("dexsim_forward_dynamics", h, env_ids, k, q, qd, &K.rows);
  if (rc) return rc;
  if ((flags & ~(DEXSIM_FD_GRAVITY | DEXSIM_FD_ARMATURE)) != 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_forward_dynamics: unknown flag bits (DEXSIM_FD_GRAVITY and DEXSIM_FD_ARMATURE are the flags)");
  if ((rc = kin_out("dexsim_forward_dynamics", "qdd", qdd, 4))) return rc;
  NEED_BOUND(h);
  K.qd = qd; K.rhs = tau; K.out = qdd; K.nrhs = 1; K.gravity = flags & DEXSIM_FD_GRAVITY; K.armature = flags & DEXSIM_FD_ARMATURE;
  KIN_LAUNCH(k_kin_fwddyn<true>, 1, K);
  return DEXSIM_OK;
}

extern "C" int dexsim_mass_solve(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* rhs, int nrhs, int flags,
                                 float* out, void* stream) {
  FwdDyn K;
  std::memset(&K, 0, sizeof K);
  int rc = kin_rows("dexsim_mass_solve", h, env_ids, k, q, &K.rows);
  if (rc) return rc;
  if ((flags & ~DEXSIM_FD_ARMATURE) != 0) return fail(DEXSIM_ERR_ARG, "dexsim_mass_solve: unknown flag bits (DEXSIM_FD_ARMATURE is the only flag)");
  if (nrhs < 1 || nrhs > DEXSIM_MSOLVE_MAX_RHS) return fail(DEXSIM_ERR_ARG, "dexsim_mass_solve: nrhs must be in [1, DEXSIM_MSOLVE_MAX_RHS]");
  if (!rhs) return fail(DEXSIM_ERR_ARG, "dexsim_mass_solve: rhs must not be NULL");
  if ((rc = kin_out("dexsim_mass_solve", "out", out, 4))) return rc;
  NEED_BOUND(h);
  K.rhs = rhs; K.out = out; K.nrhs = nrhs; K.armature = flags & DEXSIM_FD_ARMATURE;
  KIN_LAUNCH(k_kin_fwddyn<false>, 1, K);
  return DEXSIM_OK;
}

// ------------------------------------------------------------------------------------------------- dynamics derivatives
// Behind the forward dynamics: the forward route launches k_kin_fwddyn on either side of the derivative kernel.
// clang-format off
#include "dexsim_dynderiv.hip.inc"
// clang-format on

// the checks of the derivative outputs: at least one, each 4-byte aligned
static int kin_deriv_outs(const char* who, const char* na, const float* a, const char* nb, const float* b) {
  if (!a && !b) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": at least one of " + na + " and " + nb + " is required").c_str());
  int rc;
  if (a && (rc = kin_out(who, na, a, 4))) return rc;
  if (b && (rc = kin_out(who, nb, b, 4))) return rc;
  return DEXSIM_OK;
}

extern "C" int dexsim_inverse_dynamics_derivatives(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd,
                                                   const float* qdd, int flags, float* dtau_dq, float* dtau_dqd, void* stream) {
  IdDeriv K;
  std::memset(&K, 0, sizeof K);
  int rc = kin_rows_qd("dexsim_inverse_dynamics_derivatives", h, env_ids, k, q, qd, &K.rows);
  if (rc) return rc;
  if ((flags & ~DEXSIM_ID_GRAVITY) != 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_inverse_dynamics_derivatives: unknown flag bits (DEXSIM_ID_GRAVITY is the only flag)");
  if ((rc = kin_deriv_outs("dexsim_inverse_dynamics_derivatives", "dtau_dq", dtau_dq, "dtau_dqd", dtau_dqd))) return rc;
  NEED_BOUND(h);
  K.qd = qd; K.qdd = qdd; K.dq = dtau_dq; K.dqd = dtau_dqd; K.gravity = flags & DEXSIM_ID_GRAVITY;
  KIN_LAUNCH(k_kin_id_deriv<false>, 1, K);
  return DEXSIM_OK;
}

// Three launches on the caller's stream: qdd, then -d tau / d (q, qd) at that qdd, then the mass solve of the 26 rows of each
// derivative, in place.
extern "C" int dexsim_forward_dynamics_derivatives(dexsim_t h, const int64_t* env_ids, int k, const float* q, const float* qd,
                                                   const float* tau, int flags, float* qdd, float* dqdd_dq, float* dqdd_dqd, void* stream) {
  FwdDyn F;
  std::memset(&F, 0, sizeof F);
  int rc = kin_rows_qd("dexsim_forward_dynamics_derivatives", h, env_ids, k, q, qd, &F.rows);
  if (rc) return rc;
  if ((flags & ~(DEXSIM_FD_GRAVITY | DEXSIM_FD_ARMATURE)) != 0)
    return fail(DEXSIM_ERR_ARG,
                "dexsim_forward_dynamics_derivatives: unknown flag bits (DEXSIM_FD_GRAVITY and DEXSIM_FD_ARMATURE are the flags)");
  if ((rc = kin_out("dexsim_forward_dynamics_derivatives", "qdd", qdd, 4))) return rc;
  if ((rc = kin_deriv_outs("dexsim_forward_dynamics_derivatives", "dqdd_dq", dqdd_dq, "dqdd_dqd", dqdd_dqd))) return rc;
  NEED_BOUND(h);
  F.qd = qd; F.rhs = tau; F.out = qdd; F.nrhs = 1; F.gravity = flags & DEXSIM_FD_GRAVITY; F.armature = flags & DEXSIM_FD_ARMATURE;
  KIN_LAUNCH(k_kin_fwddyn<true>, 1, F);
  IdDeriv K;
  std::memset(&K, 0, sizeof K);
  K.rows = F.rows; K.qd = qd; K.qdd = qdd; K.dq = dqdd_dq; K.dqd = dqdd_dqd; K.gravity = flags & DEXSIM_FD_GRAVITY;
  KIN_LAUNCH(k_kin_id_deriv<true>, 1, K);
  static_assert(DEXSIM_NJ <= DEXSIM_MSOLVE_MAX_RHS, "the mass solve takes a derivative's 26 rows in one call");
  F.qd = nullptr; F.nrhs = DEXSIM_NJ; F.gravity = 0;
  for (float* d : {dqdd_dq, dqdd_dqd}) {
    if (!d) continue;
    F.rhs = d; F.out = d;
    KIN_LAUNCH(k_kin_fwddyn<false>, 1, F);
  }
  return DEXSIM_OK;
}
