// dexsim.hip -- libdexsim's step unit: the C-ABI (include/dexsim.h) of the simulation itself over the gfx950 step kernels
// (dexsim_physics, dexsim_l2, dexsim_state), and the library's one error record.
//
// The library is two translation units, this one and dexsim_queries.hip (the query kernels and their entry points), and neither
// includes the other's .hip.inc files: the step kernels' code is a function of this unit alone, whatever the query unit gains,
// and an edit of a query file does not recompile them.  What both need is in dexsim_device.h and dexsim_host.h.
// Build (build.py): hipcc <CODEGEN_FLAGS> -fPIC -c each unit, then hipcc --offload-arch=gfx950 -fPIC -shared -o libdexsim.so
// the two objects, this unit's first.
// No torch types, no CUDA shims, no dual back-end: this file only targets CDNA4 through HIP.
#include <cmath>
#include <algorithm>
#include "dexsim_host.h"
#include "dexsim_stamps.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

// clang-format off
#include "dexsim_physics.hip.inc"
#include "dexsim_l2.hip.inc"
#include "dexsim_state.hip.inc"
// clang-format on

// The post block runs in the sub-step kernels' LDS behind their last body (TAIL_POST); the box wave starts its tile during the
// publication (post_pre_tasks).
static_assert(lds_map_conflict({0, (int)((POST_LDS_BYTES + 64 * sizeof(float) - 1) / (64 * sizeof(float))), LIVE_PUB | LIVE_POST}) < 0,
              "the post block's LDS does not fit into the sub-step kernels' or overlaps a region live during the publication / post block");

static thread_local std::string g_last_error;

// the error record's two writers (dexsim_host.h), shared with the query unit
int fail(int code, const char* what) {
  g_last_error = what ? what : "";
  return code;
}
int fail_hip(const char* expr, hipError_t e) {
  g_last_error = std::string(expr) + ": " + hipGetErrorString(e);
  return DEXSIM_ERR_HIP;
}

// A new control step begins: new stamp for the device-side reset gate and the parity of the contact statistics (CNT_ANY_RESET,
// CNT_CONTACTS in dexsim_device.h).  Never 0 (the counters block is zero-initialised).
static void next_stamp(DexSim* h) { h->api.stamp = h->api.stamp >= 0x3ffffffe ? 1 : h->api.stamp + 1; }

static const char* const kObsKeyNames[] = {
#define X(name, dim) #name,
    DEXSIM_OBS_KEYS(X)
#undef X
};
static const int kObsKeyDims[] = {
#define X(name, dim) dim,
    DEXSIM_OBS_KEYS(X)
#undef X
};
static const char* const kRewardNames[] = {
#define X(name) #name,
    DEXSIM_REWARD_TERMS(X)
#undef X
};

extern "C" {

int dexsim_struct_sizes(size_t out[4]) {
  out[0] = sizeof(DexHandModel); out[1] = sizeof(DexSimConfig); out[2] = sizeof(DexSimField); out[3] = sizeof(DexSimBuffers);
  return DEXSIM_OK;
}

int dexsim_arena_layout(const DexSimConfig* cfg, DexSimField* fields, int max_fields, int* n_fields, size_t* arena_words) {
  if (!cfg || !n_fields || !arena_words || cfg->num_envs <= 0) return fail(DEXSIM_ERR_ARG, "dexsim_arena_layout: bad argument");
  const size_t NS = (size_t)padded(cfg->num_envs);
  size_t off = 0;
  int n = 0;
#define X(ty, nm, nrows)                                                      \
  {                                                                           \
    if (fields) {                                                             \
      if (n >= max_fields) return fail(DEXSIM_ERR_LAYOUT, "field table too small"); \
      std::snprintf(fields[n].name, sizeof fields[n].name, "%s", #nm);        \
      fields[n].rows = (nrows);                                               \
      fields[n].is_int = std::string(#ty) == "int"; \
      fields[n].offset = off;                                                 \
    }                                                                         \
    off += (size_t)(nrows) * NS;                                              \
    n++;                                                                      \
  }
  DEXSIM_FIELDS(X)
#undef X
  *n_fields = n;
  *arena_words = off;
  return DEXSIM_OK;
}

int dexsim_obs_key_info(int i, const char** name, int* offset, int* dim) {
  if (i < 0 || i >= DEXSIM_NUM_OBS_KEYS) return fail(DEXSIM_ERR_ARG, "obs key index out of range");
  int off = 0;
  for (int k = 0; k < i; k++) off += kObsKeyDims[k];
  if (name) *name = kObsKeyNames[i];
  if (offset) *offset = off;
  if (dim) *dim = kObsKeyDims[i];
  return DEXSIM_OK;
}

int dexsim_reward_term_name(int i, const char** name) {
  if (i < 0 || i >= DEXSIM_NUM_REWARD_TERMS || !name) return fail(DEXSIM_ERR_ARG, "reward term index out of range");
  *name = kRewardNames[i];
  return DEXSIM_OK;
}

int dexsim_body_name(int i, const char** name) {
  static char names[DEXSIM_NUM_HAND_BODIES][24];
  static bool init = false;
  if (!init) {
    const char* base[7] = {"hand_mount", "ARTx_link", "ARTy_link", "ARTz_link", "ARRx_link", "ARRy_link", "right_hand_base"};
    for (int b = 0; b < 7; b++) std::snprintf(names[b], 24, "%s", base[b]);
    const char* suf[6] = {"1", "2", "3", "4", "pad", "tip"};
    for (int f = 0; f < 5; f++)
      for (int l = 0; l < 6; l++) std::snprintf(names[7 + 6 * f + l], 24, "r_f_link%d_%s", f + 1, suf[l]);
    init = true;
  }
  if (i < 0 || i >= DEXSIM_NUM_HAND_BODIES || !name) return fail(DEXSIM_ERR_ARG, "body index out of range");
  *name = names[i];
  return DEXSIM_OK;
}

static int validate_model(const DexHandModel& m) {
  for (int j = 0; j < DEXSIM_NJ; j++)
    if (m.jtype[j] != (j < 3 ? 0 : 1)) return fail(DEXSIM_ERR_ARG, "model: kernels assume joints 0-2 prismatic, 3-25 revolute");
  for (int j = 0; j < 5; j++)
    if (m.mass[j] != 0.f) return fail(DEXSIM_ERR_ARG, "model: base-chain links 0-4 must be massless (palm rides on joint 5)");
  for (int j = 0; j < 5; j++) {   // the kernels and the oracle take the base's inertial data from link 5 alone
    for (int i = 0; i < 6; i++)
      if (m.inertia[j][i] != 0.f) return fail(DEXSIM_ERR_ARG, "model: base-chain links 0-4 must have zero inertia (palm rides on joint 5)");
    for (int i = 0; i < 3; i++)
      if (m.com[j][i] != 0.f) return fail(DEXSIM_ERR_ARG, "model: base-chain links 0-4 must have a zero centre of mass (palm rides on joint 5)");
  }
  for (int j = 5; j < DEXSIM_NJ; j++)
    if (!(m.mass[j] > 0.f)) return fail(DEXSIM_ERR_ARG, "model: palm and finger links need positive mass");
  for (int c = 0; c < DEXSIM_NCAP; c++) {
    const int want = c < 3 ? 5 : 6 + 4 * ((c - 3) / 3) + 1 + (c - 3) % 3;
    if (m.cap_parent[c] != want) return fail(DEXSIM_ERR_ARG, "model: capsule c must ride on palm (c<3) or finger link (c-3)/3,(c-3)%3+1");
    if (m.cap_fslot[c] < 0 || m.cap_fslot[c] >= DEXSIM_FSLOT_BOX) return fail(DEXSIM_ERR_ARG, "model: bad capsule force slot");
  }
  if (m.site_parent[0] != 5) return fail(DEXSIM_ERR_ARG, "model: site 0 (right_hand_base) must ride on joint 5");
  for (int f = 0; f < 5; f++)
    if (m.site_parent[1 + f] != 9 + 4 * f || m.site_parent[6 + f] != 9 + 4 * f)
      return fail(DEXSIM_ERR_ARG, "model: tip/pad sites must ride on the distal joint of their finger");
  for (int j = 0; j < DEXSIM_NJ; j++)
    if (!(m.hi[j] > m.lo[j])) return fail(DEXSIM_ERR_ARG, "model: joint range must be non-empty");
  return DEXSIM_OK;
}

int dexsim_create(const DexSimConfig* cfg, const DexHandModel* model, int device, dexsim_t* out) {
  if (!cfg || !model || !out) return fail(DEXSIM_ERR_ARG, "dexsim_create: null argument");
  if (cfg->num_envs <= 0 || cfg->substeps <= 0 || !(cfg->dt > 0.f)) return fail(DEXSIM_ERR_ARG, "dexsim_create: bad num_envs/substeps/dt");
  if (cfg->num_obs <= 0 || cfg->n_obs_seg <= 0 || cfg->n_obs_seg > DEXSIM_MAX_OBS_SEG) return fail(DEXSIM_ERR_ARG, "dexsim_create: bad observation table");
  if (cfg->num_actions != 6 * (cfg->policy_controls_base != 0) + 12 * (cfg->policy_controls_fingers != 0) || cfg->num_actions == 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_create: num_actions inconsistent with policy_controls_*");
  if (cfg->has_box && !(cfg->box_size > 0.f && (cfg->box_mass > 0.f || cfg->box_fixed))) return fail(DEXSIM_ERR_ARG, "dexsim_create: bad box");
  if (cfg->box_fixed && !cfg->has_box) return fail(DEXSIM_ERR_ARG, "dexsim_create: box_fixed needs has_box");
  if (cfg->dr_enabled) {   // the per-env draw reaches 1 / box_mass and the friction cones unchecked
    if (!std::isfinite(cfg->dr_mass_lo) || !std::isfinite(cfg->dr_mass_hi))
      return fail(DEXSIM_ERR_ARG, "dexsim_create: dr_mass_lo / dr_mass_hi must be finite");
    if (!std::isfinite(cfg->dr_mu_lo) || !std::isfinite(cfg->dr_mu_hi))
      return fail(DEXSIM_ERR_ARG, "dexsim_create: dr_mu_lo / dr_mu_hi must be finite");
    if (!(cfg->dr_mass_lo > 0.f)) return fail(DEXSIM_ERR_ARG, "dexsim_create: dr_mass_lo must be positive");
    if (cfg->dr_mass_lo > cfg->dr_mass_hi) return fail(DEXSIM_ERR_ARG, "dexsim_create: dr_mass_lo exceeds dr_mass_hi");
    if (cfg->dr_mu_lo < 0.f) return fail(DEXSIM_ERR_ARG, "dexsim_create: dr_mu_lo must not be negative");
    if (cfg->dr_mu_lo > cfg->dr_mu_hi) return fail(DEXSIM_ERR_ARG, "dexsim_create: dr_mu_lo exceeds dr_mu_hi");
  }
  {
    int tot = 0;
    for (int s = 0; s < cfg->n_obs_seg; s++) {
      if (cfg->obs_seg_off[s] < 0 || cfg->obs_seg_len[s] <= 0 || cfg->obs_seg_off[s] + cfg->obs_seg_len[s] > DEXSIM_OBS_ALL_DIM)
        return fail(DEXSIM_ERR_ARG, "dexsim_create: observation segment out of range");
      tot += cfg->obs_seg_len[s];
    }
    if (tot != cfg->num_obs) return fail(DEXSIM_ERR_ARG, "dexsim_create: num_obs != sum of segments");
    /* segments may repeat rows, but obs_col_row (and its staged copy in k_post) has DEXSIM_OBS_ALL_DIM entries */
    if (tot > DEXSIM_OBS_ALL_DIM) return fail(DEXSIM_ERR_ARG, "dexsim_create: more observations than the column table holds");
  }
  int rc = validate_model(*model);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DEXSIM_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(DEXSIM_ERR_NO_DEVICE, "device index out of range");
  DeviceGuard guard(device);
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != device) return fail(DEXSIM_ERR_HIP, "dexsim_create: cannot select the device");
  DexSim* h = new DexSim();
  struct Cleanup {   // a failure below must not leak the handle, the parameter block or the events
    DexSim* h; bool armed = true;
    ~Cleanup() {
      if (!armed) return;
      if (h->d_params) (void)hipFree(h->d_params);
      if (h->ev0) (void)hipEventDestroy(h->ev0);
      if (h->ev1) (void)hipEventDestroy(h->ev1);
      delete h;
    }
  } cleanup{h};
  h->cfg = *cfg; h->model = *model; h->device = device;
  h->api.stamp = 1;
  h->N = cfg->num_envs; h->NS = padded(cfg->num_envs);
  h->bound = false;
  DevParams hp;
  hp.cfg = *cfg; hp.model = *model;
  hp.h = cfg->dt / (float)cfg->substeps;
  hp.box_inv_I_k = cfg->has_box ? 6.f / (cfg->box_size * cfg->box_size) : 0.f;
  hp.obs_div_magic = (unsigned)((0x100000000ull + (unsigned long long)cfg->num_obs - 1) / (unsigned long long)cfg->num_obs);
  {   // base-chain constants (double precision on the host): see base_chain()
    struct Qd { double x, y, z, w; };
    auto qmul = [](Qd a, Qd b) {
      return Qd{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
                a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
    };
    auto qrot = [&](Qd q, const double* v, double* out) {   // R(q) v
      const Qd p{v[0], v[1], v[2], 0.0}, c{-q.x, -q.y, -q.z, q.w};
      const Qd r = qmul(qmul(q, p), c);
      out[0] = r.x; out[1] = r.y; out[2] = r.z;
    };
    Qd qc{model->spawn_quat[0], model->spawn_quat[1], model->spawn_quat[2], model->spawn_quat[3]};
    double oc[3] = {model->spawn_pos[0], model->spawn_pos[1], model->spawn_pos[2]};
    for (int j = 0; j < 4; j++) {
      const double poff[3] = {model->jpoff[j][0], model->jpoff[j][1], model->jpoff[j][2]};
      const double ax[3] = {model->jaxis[j][0], model->jaxis[j][1], model->jaxis[j][2]};
      double d[3], aw[3];
      qrot(qc, poff, d);
      for (int i = 0; i < 3; i++) oc[i] += d[i];
      const Qd qz = qmul(qc, Qd{model->jqoff[j][0], model->jqoff[j][1], model->jqoff[j][2], model->jqoff[j][3]});
      qrot(qz, ax, aw);
      for (int i = 0; i < 3; i++) { hp.base_A[j][i] = (float)aw[i]; hp.base_Oc[j][i] = (float)oc[i]; }
      qc = qz;   // prismatic joints keep the orientation; for joint 3 this is the frame at q3 = 0
    }
    hp.base_Q3z[0] = (float)qc.x; hp.base_Q3z[1] = (float)qc.y; hp.base_Q3z[2] = (float)qc.z; hp.base_Q3z[3] = (float)qc.w;
  }
  {   // hand-level broadphase radius: chain of joint offsets from the palm to the capsule's joint + capsule extent + radius
    auto len3 = [](const float* v) { return std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); };
    double reach = 0.0;
    for (int c = 0; c < DEXSIM_NCAP; c++) {
      const int j = model->cap_parent[c];
      double d = std::max(len3(model->cap_p0[c]), len3(model->cap_p1[c])) + model->cap_r[c];
      if (j >= 6) for (int l = 6 + 4 * ((j - 6) / 4); l <= j; l++) d += len3(model->jpoff[l]);
      reach = std::max(reach, d);
    }
    hp.hand_reach = (float)(reach * 1.001 + 1e-4);
  }
  {
    int k = 0;
    for (int s = 0; s < cfg->n_obs_seg; s++)
      for (int i = 0; i < cfg->obs_seg_len[s]; i++) hp.obs_col_row[k++] = cfg->obs_seg_off[s] + i;
    for (; k < DEXSIM_OBS_ALL_DIM; k++) hp.obs_col_row[k] = 0;
  }
  for (int j = 0; j < DEXSIM_NJ; j++) {
    JC& c = hp.jc[j];
    std::memset(&c, 0, sizeof c);
    for (int i = 0; i < 4; i++) c.qoff[i] = model->jqoff[j][i];
    for (int i = 0; i < 3; i++) { c.poff[i] = model->jpoff[j][i]; c.axis[i] = model->jaxis[j][i]; c.com[i] = model->com[j][i]; }
    for (int i = 0; i < 6; i++) c.inertia[i] = model->inertia[j][i];
    c.mass = model->mass[j]; c.kp = model->kp[j]; c.kd = model->kd[j]; c.armature = model->armature[j];
    c.lo = model->lo[j]; c.hi = model->hi[j];
  }
  hp.inertia_diag = 1;
  for (int j = 6; j < DEXSIM_NJ; j++)
    for (int i = 3; i < 6; i++) if (model->inertia[j][i] != 0.f) hp.inertia_diag = 0;
  {   // structural zeros and ones of the model, by exact comparison: the specialised chain forms (MS kernels, see base_chain())
    auto is3 = [](const float* v, float x, float y, float z) { return v[0] == x && v[1] == y && v[2] == z; };
    auto qoff_identity = [&](int j) { return is3(model->jqoff[j], 0.f, 0.f, 0.f) && model->jqoff[j][3] == 1.f; };
    bool ms = true;
    for (int j = 4; j < 6; j++)   // frames 4 and 5 sit on frame 3 (co-located origins), axes +e_y and +e_z
      ms = ms && qoff_identity(j) && is3(model->jpoff[j], 0.f, 0.f, 0.f) && is3(model->jaxis[j], 0.f, j == 4 ? 1.f : 0.f, j == 5 ? 1.f : 0.f);
    for (int j = 0; j < 3; j++)   // world axes of the prismatic joints: exactly e_x, e_y, e_z
      ms = ms && is3(hp.base_A[j], j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f);
    for (int j = 6; j < DEXSIM_NJ; j++)   // flexion joints (1-3 of every finger): axis +-e_y
      if ((j - 6) % 4 >= 1) ms = ms && model->jaxis[j][0] == 0.f && std::fabs(model->jaxis[j][1]) == 1.f && model->jaxis[j][2] == 0.f;
    const char* gen = std::getenv("DEXSIM_GENERAL_MODEL_PATH");   // read once, here: "1" runs the general forms for any model
    h->model_struct = ms && !(gen && gen[0] == '1');
  }
  HIP_TRY(hipMalloc(&h->d_params, sizeof(DevParams)));
  HIP_TRY(hipMemcpy(h->d_params, &hp, sizeof(DevParams), hipMemcpyHostToDevice));
  const void* const big_lds_kernels[] = {
      reinterpret_cast<const void*>(&k_solve), reinterpret_cast<const void*>(&k_post),
      reinterpret_cast<const void*>(&k_physics4<false, false>), reinterpret_cast<const void*>(&k_physics4<true, false>),
      reinterpret_cast<const void*>(&k_physics1<false, false>), reinterpret_cast<const void*>(&k_physics1<true, false>),
      reinterpret_cast<const void*>(&k_physics4<false, true>), reinterpret_cast<const void*>(&k_physics4<true, true>),
      reinterpret_cast<const void*>(&k_physics1<false, true>), reinterpret_cast<const void*>(&k_physics1<true, true>)};
  for (const void* k : big_lds_kernels) HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, FS_LDS_BYTES));
  HIP_TRY(hipEventCreate(&h->ev0));
  HIP_TRY(hipEventCreate(&h->ev1));
  cleanup.armed = false;
  *out = h;
  return DEXSIM_OK;
}

int dexsim_destroy(dexsim_t h) {
  if (!h) return DEXSIM_OK;
  DeviceGuard guard(h->device);
  (void)hipFree(h->d_params);
  (void)hipEventDestroy(h->ev0);
  (void)hipEventDestroy(h->ev1);
  if (h->tev[0]) for (int i = 0; i < 128; i++) (void)hipEventDestroy(h->tev[i]);
  delete h;
  return DEXSIM_OK;
}

int dexsim_bind(dexsim_t h, const DexSimBuffers* b) {
  if (!h || !b) return fail(DEXSIM_ERR_ARG, "dexsim_bind: null argument");
  DeviceGuard guard(h->device);
  if (!b->arena || !b->stats || !b->counters || !b->obs_buf || !b->rew_buf || !b->reset_buf || !b->episode_step_count ||
      !b->episode_length || !b->dof_state || !b->root_state)
    return fail(DEXSIM_ERR_ARG, "dexsim_bind: arena, stats, counters, obs_buf, rew_buf, reset_buf, episode_step_count, "
                                "episode_length, dof_state and root_state are required");
  size_t off = 0;
  const size_t NS = (size_t)h->NS;
  char* base = (char*)b->arena;
#define X(ty, nm, nrows)                           \
  h->arena.nm = (ty*)(base + off * 4);           \
  off += (size_t)(nrows) * NS;
  DEXSIM_FIELDS(X)
#undef X
  h->api.obs_buf = b->obs_buf; h->api.rew_buf = b->rew_buf; h->api.reset_buf = b->reset_buf;
  h->api.episode_step_count = b->episode_step_count; h->api.episode_length = b->episode_length;
  h->api.dof_state = b->dof_state; h->api.root_state = b->root_state;
  h->api.rigid_body_states = b->rigid_body_states; h->api.contact_forces_all = b->contact_forces_all;
  h->api.full_dof_targets = b->full_dof_targets; h->api.reset_samples = b->reset_samples;
  h->api.masks = b->masks; h->api.raw_targets = b->raw_targets;
  h->api.stats = b->stats; h->api.counters = b->counters;
  HIP_TRY(hipMemcpy(&h->d_params->arena, &h->arena, sizeof(Arena), hipMemcpyHostToDevice));
  h->bound = true;
  return DEXSIM_OK;
}

#define GRID(h) dim3((h)->NS / 64), dim3(64), 0, (hipStream_t)stream

static int launch_publish(dexsim_t h, int full, void* stream) {
  k_publish<<<dim3(h->NS / 64), dim3(384), 0, (hipStream_t)stream>>>(h->arena, h->api, h->d_params, h->api.counters, full, h->NS, h->N);
  LAUNCH_CHECK();
  return DEXSIM_OK;
}
static int launch_post(dexsim_t h, int obs_only, int fold_reset, void* stream) {
  k_post<<<dim3(h->NS / 64), dim3(512), POST_LDS_BYTES, (hipStream_t)stream>>>(h->arena, h->api, h->d_params, h->api.counters, obs_only, fold_reset, h->NS, h->N);
  LAUNCH_CHECK();
  return DEXSIM_OK;
}

// LDS budget of the contact-solve kernel: stage the rows of as many contacts as fit next to u_f and the impulses.
// At <= 1 wavefront per CU (num_envs <= 64 * #CUs) the whole 160 KiB is this wave's to use.
static int solve_kstage(const DexSim* h) { return h->NS <= 64 * 256 ? 4 : 2; }   // 4: (60 + 7 KMAX + 4 x 84) words x 256 B = 141 KiB
static size_t solve_lds_bytes(int kstage) { return (size_t)SOLVE_LDS_WORDS(kstage) * 64 * sizeof(float); }

static int launch_solve(dexsim_t h, void* stream) {
  const int ks = solve_kstage(h);
  const size_t lds = solve_lds_bytes(ks);
  k_solve<<<dim3(h->NS / 64), dim3(64), lds, (hipStream_t)stream>>>(h->arena, h->d_params, h->api.counters, h->api.stamp, ks, h->NS, h->N);
  LAUNCH_CHECK();
  return DEXSIM_OK;
}
static int launch_dynamics(dexsim_t h, void* stream) {
  k_dynamics<<<dim3(h->NS / 64), dim3(384), 0, (hipStream_t)stream>>>(h->arena, h->d_params, h->NS);
  LAUNCH_CHECK();
  return DEXSIM_OK;
}

int dexsim_init_state(dexsim_t h, void* stream) {
  NEED_BOUND(h);
  size_t words = 0; int nf = 0;
  dexsim_arena_layout(&h->cfg, nullptr, 0, &nf, &words);
  HIP_TRY(hipMemsetAsync(h->arena.q, 0, words * 4, (hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(h->api.episode_step_count, 0, sizeof(int64_t) * h->N, (hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(h->api.episode_length, 0, sizeof(int64_t) * h->N, (hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(h->api.reset_buf, 0, h->N, (hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(h->api.rew_buf, 0, sizeof(float) * h->N, (hipStream_t)stream));
  h->api.stamp = 1;
  k_init<<<GRID(h)>>>(h->arena, h->api, h->d_params, h->NS, h->N);
  LAUNCH_CHECK();
  return launch_publish(h, 0, stream);
}

int dexsim_process_actions(dexsim_t h, const float* actions, int zero_targets, void* stream) {
  NEED_BOUND(h);
  if (!actions) return fail(DEXSIM_ERR_ARG, "Actions cannot be None");   // action_processor.py:296-297
  next_stamp(h);   // the action stage opens a control step
  ApiPtrs api = h->api;
  if (api.actions_copy == actions) api.actions_copy = nullptr;   // the caller passed the bound copy itself: nothing to copy
  k_actions<<<dim3(h->NS / 64), dim3(384), 0, (hipStream_t)stream>>>(h->arena, api, h->d_params, actions, zero_targets, h->NS, h->N);
  LAUNCH_CHECK();
  return DEXSIM_OK;
}

// One physics step: substeps / 4 launches of k_physics4, then substeps % 4 of k_physics1.  The action block rides on the first
// launch, `tail` (TAIL_POST: the post-physics block, ungated; TAIL_RESET: phase 1 of the in-step reset + the step statistics, gated)
// on the last; the launches before the last carry TAIL_NOT_FINAL (their last body does not add to the contact statistics).
static int physics_step(dexsim_t h, int gate_on_reset, int tail, void* stream, const float* actions = nullptr) {
  const size_t lds = FS_LDS_BYTES;
  const dim3 grid(h->NS / 64), block(448);
  const int n4 = h->cfg.substeps / 4, n = n4 + h->cfg.substeps % 4;
  for (int i = 0; i < n; i++) {
    const int t = i == n - 1 ? tail : TAIL_NOT_FINAL;
    const float* act = i == 0 ? actions : nullptr;
    ApiPtrs api = h->api;
    if (api.actions_copy == act) api.actions_copy = nullptr;   // `act` is __restrict__: never alias it with the copy sink
    auto* k = h->model_struct ? (i < n4 ? (gate_on_reset ? k_physics4<true, true> : k_physics4<false, true>) : (gate_on_reset ? k_physics1<true, true> : k_physics1<false, true>))
                              : (i < n4 ? (gate_on_reset ? k_physics4<true, false> : k_physics4<false, false>) : (gate_on_reset ? k_physics1<true, false> : k_physics1<false, false>));
    k<<<grid, block, lds, (hipStream_t)stream>>>(h->arena, api, h->d_params, h->api.counters, act, t, h->NS, h->N);
    LAUNCH_CHECK();
  }
  return DEXSIM_OK;
}

int dexsim_physics_step(dexsim_t h, int gate_on_reset, void* stream) {
  NEED_BOUND(h);
  return physics_step(h, gate_on_reset, 0, stream);
}

int dexsim_post_physics(dexsim_t h, int obs_only, void* stream) {
  NEED_BOUND(h);
  // fold_reset: phase 0 of the in-step reset runs inside k_post
  const int rc = launch_post(h, obs_only, !obs_only, stream);
  if (rc || obs_only) return rc;
  // reset_idx(nonzero(reset_buf)) incl. the extra physics step for ALL envs (step_processor.py:109-111,
  // reset_manager.py:180), gated on the device-side flag instead of torch.any() on the host; phase 1 + statistics run in its
  // last launch
  return physics_step(h, 1, TAIL_RESET, stream);
}

int dexsim_step(dexsim_t h, const float* actions, void* stream) {
  NEED_BOUND(h);
  // actions + physics + post-physics (+ phase 0 of the in-step reset) in the ungated half, then the device-gated extra
  // physics step with phase 1 of the reset and the step statistics: with substeps == 4 a control step is 2 launches
  if (!actions) return fail(DEXSIM_ERR_ARG, "Actions cannot be None");   // action_processor.py:296-297
  next_stamp(h);
  h->last_actions = actions;
  const int slot = h->timing ? ((h->timing - 1) & 63) : -1;
  if (slot >= 0) HIP_TRY(hipEventRecord(h->tev[2 * slot], (hipStream_t)stream));
  int rc = physics_step(h, 0, TAIL_POST, stream, actions);
  if (rc) return rc;
  if (slot >= 0) { HIP_TRY(hipEventRecord(h->tev[2 * slot + 1], (hipStream_t)stream)); h->timing++; }
  return physics_step(h, 1, TAIL_RESET, stream);
}

int dexsim_reset_idx(dexsim_t h, const int64_t* env_ids, int k, void* stream) {
  NEED_BOUND(h);
  if (k == 0) return DEXSIM_OK;   // dexhand_base.py:746-747
  if (k < 0 || (!env_ids && k != h->N)) return fail(DEXSIM_ERR_ARG, "dexsim_reset_idx: bad env_ids");
  const int mode = env_ids ? 1 : 2;
  dim3 grid((k + 63) / 64);
  k_reset<<<grid, 64, 0, (hipStream_t)stream>>>(h->arena, h->api, h->d_params, env_ids, k, mode, 0, h->NS, h->N);
  LAUNCH_CHECK();
  int rc = dexsim_physics_step(h, 0, stream);
  if (rc) return rc;
  k_reset<<<grid, 64, 0, (hipStream_t)stream>>>(h->arena, h->api, h->d_params, env_ids, k, mode, 1, h->NS, h->N);
  LAUNCH_CHECK();
  return DEXSIM_OK;
}

int dexsim_reset(dexsim_t h, void* stream) {
  NEED_BOUND(h);
  next_stamp(h);
  k_begin_step<<<1, 64, 0, (hipStream_t)stream>>>(h->api.counters, h->api.stamp);
  LAUNCH_CHECK();
  int rc = dexsim_reset_idx(h, nullptr, h->N, stream);
  if (rc) return rc;
  rc = dexsim_post_physics(h, 1, stream);
  if (rc) return rc;
  return dexsim_post_physics(h, 0, stream);
}

int dexsim_refresh_body_states(dexsim_t h, void* stream) {
  NEED_BOUND(h);
  if (!h->api.rigid_body_states || !h->api.contact_forces_all) return fail(DEXSIM_ERR_NOT_BOUND, "rigid_body_states / contact_forces_all not bound");
  return launch_publish(h, 1, stream);
}

static int ingest(dexsim_t h, const int64_t* ids, int k, int what, void* stream) {
  NEED_BOUND(h);
  if (k == 0) return DEXSIM_OK;
  if (!ids || k < 0) return fail(DEXSIM_ERR_ARG, "indexed set: bad env_ids");
  k_ingest<<<dim3((k + 63) / 64), 64, 0, (hipStream_t)stream>>>(h->arena, h->api, h->d_params, ids, k, what, h->NS, h->N);
  LAUNCH_CHECK();
  return launch_publish(h, 0, stream);
}
int dexsim_set_dof_state_indexed(dexsim_t h, const int64_t* env_ids, int k, void* stream) { return ingest(h, env_ids, k, 0, stream); }
int dexsim_set_root_state_indexed(dexsim_t h, const int64_t* env_ids, int k, void* stream) { return ingest(h, env_ids, k, 1, stream); }

static int launch_stage(dexsim_t h, int stage, void* stream) {
  if (h->cfg.joint_limit_rows && (stage == DEXSIM_STAGE_DYNAMICS || stage == DEXSIM_STAGE_SOLVE))
    return fail(DEXSIM_ERR_ARG, "the un-fused k_dynamics / k_solve test kernels do not build joint-limit rows (joint_limit_rows): use the fused path");
  switch (stage) {
    case DEXSIM_STAGE_DYNAMICS: return launch_dynamics(h, stream);
    case DEXSIM_STAGE_SOLVE: return launch_solve(h, stream);
    case DEXSIM_STAGE_PUBLISH: return launch_publish(h, 0, stream);
    case DEXSIM_STAGE_SUBSTEP:   // one sub-step as its own launch, counting its contacts
      (h->model_struct ? k_physics1<false, true> : k_physics1<false, false>)<<<dim3(h->NS / 64), dim3(448), FS_LDS_BYTES, (hipStream_t)stream>>>(
          h->arena, h->api, h->d_params, h->api.counters, nullptr, 0, h->NS, h->N);
      break;
    case DEXSIM_STAGE_PHYSICS: return physics_step(h, 0, 0, stream);
    case DEXSIM_STAGE_STEP:   // the ungated half of dexsim_step: actions + all sub-steps + post-physics, same arguments
      if (!h->last_actions) return fail(DEXSIM_ERR_ARG, "DEXSIM_STAGE_STEP needs a previous dexsim_step");
      return physics_step(h, 0, TAIL_POST, stream, h->last_actions);
    case DEXSIM_STAGE_POST: return launch_post(h, 0, 0, stream);
    case DEXSIM_STAGE_POST + 100: return launch_post(h, 1, 0, stream);
    case DEXSIM_STAGE_RESET:   // both phases for the flagged envs, without the device-side gate and without physics
      k_reset<<<GRID(h)>>>(h->arena, h->api, h->d_params, nullptr, 0, 3, 0, h->NS, h->N);
      k_reset<<<GRID(h)>>>(h->arena, h->api, h->d_params, nullptr, 0, 3, 1, h->NS, h->N);
      break;
    case DEXSIM_STAGE_FINALIZE:   // closes a staged control step and opens the next one
      k_finalize<<<1, 64, 0, (hipStream_t)stream>>>(h->api, h->d_params, h->N);
      next_stamp(h);
      k_begin_step<<<1, 64, 0, (hipStream_t)stream>>>(h->api.counters, h->api.stamp);
      break;
    default: return fail(DEXSIM_ERR_ARG, "unknown stage");
  }
  LAUNCH_CHECK();
  return DEXSIM_OK;
}

int dexsim_run_stage(dexsim_t h, int stage, void* stream) {
  NEED_BOUND(h);
  return launch_stage(h, stage, stream);
}

int dexsim_time_stage(dexsim_t h, int stage, int launches, void* stream, float* mean_us) {
  NEED_BOUND(h);
  if (launches <= 0 || !mean_us) return fail(DEXSIM_ERR_ARG, "dexsim_time_stage: bad argument");
  double total = 0;
  for (int i = 0; i < launches; i++) {
    // keep the state physical: every timed solve is preceded by its (untimed) dynamics launch
    if (stage == DEXSIM_STAGE_SOLVE) { int rc = launch_stage(h, DEXSIM_STAGE_DYNAMICS, stream); if (rc) return rc; }
    HIP_TRY(hipEventRecord(h->ev0, (hipStream_t)stream));
    int rc = launch_stage(h, stage, stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev1, (hipStream_t)stream));
    HIP_TRY(hipEventSynchronize(h->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    total += ms;
  }
  *mean_us = (float)(total * 1000.0 / launches);
  return DEXSIM_OK;
}

int dexsim_begin_step(dexsim_t h, void* stream) {
  NEED_BOUND(h);
  next_stamp(h);
  k_begin_step<<<1, 64, 0, (hipStream_t)stream>>>(h->api.counters, h->api.stamp);
  LAUNCH_CHECK();
  return DEXSIM_OK;
}

int dexsim_set_step_sink(dexsim_t h, float* obs, float* rew, uint8_t* done) {
  if (!h) return fail(DEXSIM_ERR_ARG, "null handle");
  h->api.sink_obs = obs; h->api.sink_rew = rew; h->api.sink_done = done;   // kernel arguments: effective from the next launch
  return DEXSIM_OK;
}

int dexsim_set_obs_dict_mode(dexsim_t h, int mode) {
  if (!h) return fail(DEXSIM_ERR_ARG, "null handle");
  if (mode != 0 && mode != 1) return fail(DEXSIM_ERR_ARG, "dexsim_set_obs_dict_mode: mode must be 0 (all rows) or 1 (policy keys only)");
  h->api.skip_obs_all = mode;   // kernel argument: effective from the next launch
  return DEXSIM_OK;
}

int dexsim_set_phase_probe(dexsim_t h, uint32_t* buf) {
  if (!h) return fail(DEXSIM_ERR_ARG, "null handle");
  h->api.probe = buf;   // kernel argument: effective from the next launch
  return DEXSIM_OK;
}

int dexsim_set_stats_sink(dexsim_t h, float* dst) {
  if (!h) return fail(DEXSIM_ERR_ARG, "null handle");
  h->api.sink_stats = dst;   // kernel argument: effective from the next launch
  return DEXSIM_OK;
}

int dexsim_set_action_copy(dexsim_t h, float* dst) {
  if (!h) return fail(DEXSIM_ERR_ARG, "null handle");
  h->api.actions_copy = dst;
  return DEXSIM_OK;
}

int dexsim_step_timing(dexsim_t h, int enable, float* mean_us, int* n) {
  NEED_BOUND(h);
  if (enable) {
    if (!h->tev[0]) for (int i = 0; i < 128; i++) HIP_TRY(hipEventCreate(&h->tev[i]));
    h->timing = 1;
    return DEXSIM_OK;
  }
  const int rec = h->timing ? h->timing - 1 : 0;
  h->timing = 0;
  const int cnt = rec < 64 ? rec : 64;
  double tot = 0.0;
  for (int i = 0; i < cnt; i++) {
    HIP_TRY(hipEventSynchronize(h->tev[2 * i + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->tev[2 * i], h->tev[2 * i + 1]));
    tot += ms;
  }
  if (mean_us) *mean_us = cnt ? (float)(tot * 1000.0 / cnt) : 0.f;
  if (n) *n = cnt;
  return DEXSIM_OK;
}

const char* dexsim_error_string(int code) {
  switch (code) {
    case DEXSIM_OK: return "ok";
    case DEXSIM_ERR_ARG: return "invalid argument";
    case DEXSIM_ERR_NOT_BOUND: return "buffers not bound";
    case DEXSIM_ERR_HIP: return "HIP runtime error";
    case DEXSIM_ERR_NO_DEVICE: return "no usable HIP device";
    case DEXSIM_ERR_LAYOUT: return "arena layout error";
    default: return "unknown error";
  }
}

const char* dexsim_last_error(void) { return g_last_error.c_str(); }

} // extern "C"

// ------------------------------------------------------------------------------------------------- state records
// Record = [ROWS-layout state fields, in DEXSIM_STATE_FIELDS order][wlam quads][API sections]; word offsets inside a record.
struct StateLayout {
  int off_wlam, off_obs, off_rew, off_reset, off_esc, off_elen, off_dof, off_root, off_fdt, off_masks, words;
  int num_obs, root_words;
};
static StateLayout state_layout_of(const DexSimConfig& c) {
  StateLayout L;
  int o = STATE_NROWS;
  L.off_wlam = o; o += DEXSIM_ROWS_wlam;
  L.num_obs = c.num_obs; L.root_words = 13 * (1 + (c.has_box ? 1 : 0));
  L.off_obs = o; o += c.num_obs;
  L.off_rew = o; o += 1;
  L.off_reset = o; o += 1;
  L.off_esc = o; o += 2;
  L.off_elen = o; o += 2;
  L.off_dof = o; o += DEXSIM_NJ * 2;
  L.off_root = o; o += L.root_words;
  L.off_fdt = o; o += DEXSIM_NJ;
  L.off_masks = o; o += (DEXSIM_NUM_MASKS + 3) / 4;
  L.words = o;
  return L;
}

extern "C" int dexsim_state_layout(const DexSimConfig* cfg, DexSimField* fields, int max_fields, int* n_fields, size_t* record_words) {
  if (!cfg || !n_fields || !record_words || cfg->num_envs <= 0 || cfg->num_obs <= 0)
    return fail(DEXSIM_ERR_ARG, "dexsim_state_layout: bad argument");
  const StateLayout L = state_layout_of(*cfg);
  int n = 0;
  auto put = [&](const char* prefix, const char* name, int rows, int is_int, int off) {
    if (fields) {
      if (n >= max_fields) return false;
      std::snprintf(fields[n].name, sizeof fields[n].name, "%s%s", prefix, name);
      fields[n].rows = rows; fields[n].is_int = is_int; fields[n].offset = (size_t)off;
    }
    n++;
    return true;
  };
  int off = 0;
#define X(nm, layout)                                                                                                         \
  if (DEXSIM_LAYOUT_##layout == DEXSIM_LAYOUT_ROWS) {                                                                         \
    if (!put("", #nm, DEXSIM_ROWS_##nm, std::is_same<decltype(Arena::nm), int*>::value, off)) return fail(DEXSIM_ERR_LAYOUT, "field table too small"); \
    off += DEXSIM_ROWS_##nm;                                                                                                  \
  }
  DEXSIM_STATE_FIELDS(X)
#undef X
  const struct { const char* name; int rows, is_int, off; } sec[] = {
      {"wlam", DEXSIM_ROWS_wlam, 0, L.off_wlam},
      {"api.obs_buf", L.num_obs, 0, L.off_obs}, {"api.rew_buf", 1, 0, L.off_rew}, {"api.reset_buf", 1, 1, L.off_reset},
      {"api.episode_step_count", 2, 1, L.off_esc}, {"api.episode_length", 2, 1, L.off_elen},
      {"api.dof_state", DEXSIM_NJ * 2, 0, L.off_dof}, {"api.root_state", L.root_words, 0, L.off_root},
      {"api.full_dof_targets", DEXSIM_NJ, 0, L.off_fdt}, {"api.masks", (DEXSIM_NUM_MASKS + 3) / 4, 1, L.off_masks}};
  for (const auto& s : sec)
    if (!put("", s.name, s.rows, s.is_int, s.off)) return fail(DEXSIM_ERR_LAYOUT, "field table too small");
  *n_fields = n;
  *record_words = (size_t)L.words;
  return DEXSIM_OK;
}

// The three kernels of the family.
static constexpr auto k_state_save = &k_state_xfer<ST_SAVE>;   // instance -> bank
static constexpr auto k_state_load = &k_state_xfer<ST_LOAD>;   // bank -> instance
static constexpr auto k_state_copy = &k_state_xfer<ST_COPY>;   // instance -> instance (fork)

// The launch of one of them: every chunk of the record x every tile of 64 lanes.
static int state_xfer(dexsim_t h, int mode, const int64_t* src_idx, const int64_t* dst_idx, int k, long long src_lim, long long dst_lim,
                      void* bank, long long capacity, void* stream) {
  const StateLayout L = state_layout_of(h->cfg);
  StateXfer X;
  std::memset(&X, 0, sizeof X);
  X.src_idx = src_idx; X.dst_idx = dst_idx; X.k = k; X.src_lim = src_lim; X.dst_lim = dst_lim;
  X.bank = (unsigned*)bank; X.caps = (capacity + 63) / 64 * 64;
  X.n_row_chunks = (STATE_NROWS + ST_ROW_CHUNK - 1) / ST_ROW_CHUNK;
  X.n_quad_chunks = (STATE_NQUADS + ST_QUAD_CHUNK - 1) / ST_QUAD_CHUNK;
  X.off_wlam = L.off_wlam; X.off_rew = L.off_rew; X.off_reset = L.off_reset; X.off_esc = L.off_esc; X.off_elen = L.off_elen;
  X.off_masks = L.off_masks;
  const struct { float* base; int len, off; } aos[] = {{h->api.obs_buf, L.num_obs, L.off_obs}, {h->api.dof_state, DEXSIM_NJ * 2, L.off_dof},
                                                       {h->api.root_state, L.root_words, L.off_root}, {h->api.full_dof_targets, DEXSIM_NJ, L.off_fdt}};
  for (const auto& a : aos) {
    if (!a.base) continue;   // an optional API tensor that is not bound has no rows to move
    for (int c0 = 0; c0 < a.len; c0 += ST_AOS_CHUNK) {
      if (X.n_aos >= ST_MAX_AOS) return fail(DEXSIM_ERR_ARG, "state transfer: observation row too long for the AoS chunk table");
      X.aos[X.n_aos++] = StateAos{(unsigned*)a.base, a.len, c0, std::min(ST_AOS_CHUNK, a.len - c0), a.off};
    }
  }
  const dim3 grid((k + 63) / 64, X.n_row_chunks + X.n_quad_chunks + X.n_aos + 1), block(256);
  auto* kern = mode == ST_SAVE ? k_state_save : mode == ST_LOAD ? k_state_load : k_state_copy;
  kern<<<grid, block, 0, (hipStream_t)stream>>>(h->api, h->d_params, X, h->NS, h->N);
  LAUNCH_CHECK();
  return DEXSIM_OK;
}

static int state_save_load(dexsim_t h, int mode, const int64_t* env_ids, const int64_t* slots, int k, void* bank, int64_t capacity, void* stream) {
  const char* who = mode == ST_SAVE ? "dexsim_save_state" : "dexsim_load_state";
  const bool identity = !env_ids && !slots;
  if (k < 0) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": k must not be negative").c_str());
  NEED_BOUND(h);
  if (!bank) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": the state bank is NULL").c_str());
  if (((uintptr_t)bank & 15) != 0) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": the state bank must be 16-byte aligned").c_str());
  if (capacity <= 0 || capacity > 0x7fffffc0ll) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": bad capacity").c_str());
  if (identity) {
    if (capacity < h->NS) return fail(DEXSIM_ERR_ARG, (std::string(who) + ": the identity over all lanes needs capacity >= NS = pad64(num_envs)").c_str());
    k = h->NS;
  } else if (!env_ids || !slots) {
    return fail(DEXSIM_ERR_ARG, (std::string(who) + ": env_ids and slots must both be given (or both NULL: identity)").c_str());
  }
  if (k == 0) return DEXSIM_OK;
  const long long env_lim = identity ? h->NS : h->N;
  return mode == ST_SAVE ? state_xfer(h, mode, env_ids, slots, k, env_lim, capacity, bank, capacity, stream)
                         : state_xfer(h, mode, slots, env_ids, k, capacity, env_lim, bank, capacity, stream);
}

extern "C" int dexsim_save_state(dexsim_t h, const int64_t* env_ids, const int64_t* slots, int k, void* bank, int64_t capacity, void* stream) {
  return state_save_load(h, ST_SAVE, env_ids, slots, k, bank, capacity, stream);
}
extern "C" int dexsim_load_state(dexsim_t h, const int64_t* env_ids, const int64_t* slots, int k, const void* bank, int64_t capacity, void* stream) {
  return state_save_load(h, ST_LOAD, env_ids, slots, k, const_cast<void*>(bank), capacity, stream);
}

extern "C" int dexsim_copy_envs(dexsim_t h, const int64_t* src_ids, const int64_t* dst_ids, int k, void* stream) {
  if (k < 0) return fail(DEXSIM_ERR_ARG, "dexsim_copy_envs: k must not be negative");
  NEED_BOUND(h);
  if (k == 0) return DEXSIM_OK;
  if (!src_ids || !dst_ids) return fail(DEXSIM_ERR_ARG, "dexsim_copy_envs: src_ids and dst_ids are required");
  return state_xfer(h, ST_COPY, src_ids, dst_ids, k, h->N, h->N, nullptr, 0, stream);
}

extern "C" int dexsim_get_step_stamp(dexsim_t h, int* stamp) {
  if (!h) return fail(DEXSIM_ERR_ARG, "null handle");
  if (!stamp) return fail(DEXSIM_ERR_ARG, "dexsim_get_step_stamp: null argument");
  *stamp = h->api.stamp;
  return DEXSIM_OK;
}
extern "C" int dexsim_set_step_stamp(dexsim_t h, int stamp) {
  if (!h) return fail(DEXSIM_ERR_ARG, "null handle");
  if (stamp < 1 || stamp > 0x3ffffffe) return fail(DEXSIM_ERR_ARG, "dexsim_set_step_stamp: the stamp must be in [1, 0x3ffffffe]");
  h->api.stamp = stamp;
  return DEXSIM_OK;
}
