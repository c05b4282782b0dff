// dexsim_state.hip.inc -- save / load / fork of per-env simulation state (dexsim_save_state, dexsim_load_state, dexsim_copy_envs).
//
// A state record (include/dexsim.h) is the env's share of the persistent arena fields (DEXSIM_STATE_FIELDS, dexsim_device.h)
// plus its rows of the published API tensors.  Records live in the caller's state bank, slot-fastest SoA: record word w of slot s
// is bank[w * CAPS + s] (CAPS = capacity padded to 64), the quads of wlam [quad][slot][4] -- the arena's own two layouts with the
// slot in the place of the env, so that for contiguous ids every access on either side is one full-wave access to consecutive
// addresses (4 B per lane for rows, 16 B for quads).  Arbitrary ids turn the arena side into a gather; the bank side stays
// coalesced when the slots are contiguous.
//
// One kernel family, k_state_xfer<ST_SAVE | ST_LOAD | ST_COPY>: a workgroup of 4 waves moves (64 lanes) x (one chunk of the
// record): 32 arena rows, 16 wlam quads, <= 64 columns of one AoS API tensor (through an LDS transpose: lanes run along the
// env's row on the AoS side, along the slots on the bank side) or the packed 64-bit / 8-bit API words.  No atomics; LDS for
// the transpose only.  The arena is reached through DevParams::arena (scalar cache); which arena row a record row is follows from
// compile-time run bounds.  Nothing here is on the step path.

enum { ST_SAVE = 0, ST_LOAD = 1, ST_COPY = 2 };

enum {
#define X(type, name, rows) DEXSIM_FIDX_##name,
  DEXSIM_FIELDS(X)
#undef X
  DEXSIM_NFIELDS
};
static_assert(DEXSIM_FIDX_q == 0, "the arena base is the first field");

constexpr int kFieldRows[DEXSIM_NFIELDS] = {
#define X(type, name, rows) (rows),
    DEXSIM_FIELDS(X)
#undef X
};
constexpr int field_row0(int f) { int o = 0; for (int i = 0; i < f; i++) o += kFieldRows[i]; return o; }

// record rows of the ROWS-layout state fields and quads of the QUAD-layout ones (wlam is the only one)
constexpr int STATE_NROWS = 0
#define X(name, layout) + (DEXSIM_LAYOUT_##layout == DEXSIM_LAYOUT_ROWS ? (int)DEXSIM_ROWS_##name : 0)
    DEXSIM_STATE_FIELDS(X)
#undef X
    ;
constexpr int STATE_NQUAD_FIELDS = 0
#define X(name, layout) + (DEXSIM_LAYOUT_##layout == DEXSIM_LAYOUT_QUAD ? 1 : 0)
    DEXSIM_STATE_FIELDS(X)
#undef X
    ;
static_assert(DEXSIM_ROWS_wlam % (4 * 16) == 0, "the quads of wlam are moved in whole chunks of ST_QUAD_CHUNK");
static_assert(STATE_NQUAD_FIELDS == 1, "k_state_xfer moves exactly one quad-layout field (wlam)");
constexpr int STATE_NQUADS = DEXSIM_ROWS_wlam / 4;

// record row -> arena row (the arena is one [row][env] matrix from its first field on).  The persistent fields form a few runs of
// consecutive arena rows; their bounds are compile-time constants, so the mapping is a handful of scalar compares on immediates:
// no table in memory, no load in front of the field accesses.
#define ST_MAX_RUNS 8
struct StateRuns { int n; int rec0[ST_MAX_RUNS], arena0[ST_MAX_RUNS]; };
constexpr StateRuns make_state_runs() {
  StateRuns t{};
  int rec = 0, end = -1;
#define X(name, layout)                                                                   \
  if (DEXSIM_LAYOUT_##layout == DEXSIM_LAYOUT_ROWS) {                                     \
    const int a0 = field_row0(DEXSIM_FIDX_##name);                                        \
    if (a0 != end) { t.rec0[t.n] = rec; t.arena0[t.n] = a0; t.n++; }                      \
    rec += (int)DEXSIM_ROWS_##name; end = a0 + (int)DEXSIM_ROWS_##name;                   \
  }
  DEXSIM_STATE_FIELDS(X)
#undef X
  return t;
}
static_assert(make_state_runs().n <= ST_MAX_RUNS, "DEXSIM_STATE_FIELDS: more runs of consecutive arena fields than ST_MAX_RUNS "
                                                  "(list the fields in DEXSIM_FIELDS order)");
__device__ __forceinline__ unsigned state_arena_row(int r) {
  constexpr StateRuns R = make_state_runs();
  unsigned a = (unsigned)(R.arena0[0] + r);
#pragma unroll
  for (int i = 1; i < R.n; i++) if (r >= R.rec0[i]) a = (unsigned)(R.arena0[i] + (r - R.rec0[i]));
  return a;
}

#define ST_ROW_CHUNK 32    /* arena rows per workgroup: 8 independent 4-byte accesses per lane and wave */
#define ST_QUAD_CHUNK 16   /* wlam quads per workgroup: 4 independent 16-byte accesses per lane and wave */
#define ST_AOS_CHUNK 64    /* columns of an AoS API tensor per workgroup (one 64 x 64 LDS tile, rows padded to 65 words) */
#define ST_MAX_AOS 12
#define ST_MISC_WORDS 9    /* rew, reset, episode_step_count lo/hi, episode_length lo/hi, masks packed 4 bytes per word */
static_assert(DEXSIM_NUM_MASKS <= 12, "the mask column of an env is packed into 3 record words");

struct StateAos {   // <= ST_AOS_CHUNK columns [col0, col0 + ncols) of an (N, L) AoS API tensor; record rows rec_off + col0 + c
  unsigned* base; int L, col0, ncols, rec_off;
};
struct StateXfer {
  const int64_t* src_idx;   // per lane: env id (instance side) or slot (bank side) to read; NULL = the lane itself
  const int64_t* dst_idx;   // ... to write
  int k;                    // lanes
  long long src_lim, dst_lim;   // lanes whose index is outside [0, lim) move nothing (never an out-of-bounds access)
  unsigned* bank; long long caps;
  int n_row_chunks, n_quad_chunks, n_aos;
  int off_wlam, off_rew, off_reset, off_esc, off_elen, off_masks;   // record word offsets
  StateAos aos[ST_MAX_AOS];
};

template <int MODE>
__global__ __launch_bounds__(256) void k_state_xfer(ApiPtrs T, const DevParams* __restrict__ P, StateXfer X, int NS, int NR) {
  constexpr bool SRC_BANK = MODE == ST_LOAD, DST_BANK = MODE == ST_SAVE;
  __shared__ unsigned s_tile[ST_AOS_CHUNK * 65];
  __shared__ int s_si[64], s_di[64];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l = blockIdx.x * 64 + lane;
  long long si = -1, di = -1;
  if (l < X.k) { si = X.src_idx ? X.src_idx[l] : l; di = X.dst_idx ? X.dst_idx[l] : l; }
  const bool act = si >= 0 && si < X.src_lim && di >= 0 && di < X.dst_lim;
  const size_t caps = (size_t)X.caps, ns = (size_t)NS;
  unsigned* const arena = (unsigned*)P->arena.q;
  int y = blockIdx.y;

  if (y < X.n_row_chunks) {   // ---------------------------------------------------------------- arena rows
    // a wave moves 8 consecutive record rows; the row index is wave-uniform, so the arena row and the row's base address are
    // scalar arithmetic.  All loads are issued before the first store (rows past the end re-read the last row and are not stored).
    const int r0 = y * ST_ROW_CHUNK + wv * (ST_ROW_CHUNK / 4);
    if (act && r0 < STATE_NROWS) {
      unsigned v[ST_ROW_CHUNK / 4], ar[ST_ROW_CHUNK / 4];
#pragma unroll
      for (int i = 0; i < ST_ROW_CHUNK / 4; i++) ar[i] = state_arena_row(min(r0 + i, STATE_NROWS - 1));
#pragma unroll
      for (int i = 0; i < ST_ROW_CHUNK / 4; i++) {
        const int r = min(r0 + i, STATE_NROWS - 1);
        const unsigned* sp = SRC_BANK ? X.bank + (size_t)r * caps : arena + (size_t)ar[i] * ns;
        v[i] = GPTR(sp)[si];
      }
#pragma unroll
      for (int i = 0; i < ST_ROW_CHUNK / 4; i++) {
        const int r = r0 + i;
        if (r < STATE_NROWS) {
          unsigned* dp = DST_BANK ? X.bank + (size_t)r * caps : arena + (size_t)ar[i] * ns;
          GPTR(dp)[di] = v[i];
        }
      }
    }
    return;
  }
  y -= X.n_row_chunks;

  if (y < X.n_quad_chunks) {   // --------------------------------------------------------------- wlam quads
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    u4* const aq = (u4*)P->arena.wlam;
    u4* const bq = (u4*)(X.bank + (size_t)X.off_wlam * caps);
    const int q0 = y * ST_QUAD_CHUNK + wv * (ST_QUAD_CHUNK / 4);
    if (act) {
      u4 v[ST_QUAD_CHUNK / 4];
#pragma unroll
      for (int i = 0; i < ST_QUAD_CHUNK / 4; i++) v[i] = GPTR(SRC_BANK ? bq + (size_t)(q0 + i) * caps : aq + (size_t)(q0 + i) * ns)[si];
#pragma unroll
      for (int i = 0; i < ST_QUAD_CHUNK / 4; i++) GPTR(DST_BANK ? bq + (size_t)(q0 + i) * caps : aq + (size_t)(q0 + i) * ns)[di] = v[i];
    }
    return;
  }
  y -= X.n_quad_chunks;

  // the API sections exist for real envs only (padded lanes own arena fields, never API rows)
  const bool act_api = act && (SRC_BANK || si < NR) && (DST_BANK || di < NR);

  if (y < X.n_aos) {   // ----------------------------------------------------------------------- AoS API tensors
    const StateAos a = X.aos[y];
    if (wv == 0) { s_si[lane] = act_api ? (int)si : -1; s_di[lane] = act_api ? (int)di : -1; }
    __syncthreads();
    const int total = 64 * a.ncols;
    if (SRC_BANK) {
      for (int c = wv; c < a.ncols; c += 4)
        if (act_api) s_tile[c * 65 + lane] = GPTR(X.bank)[(size_t)(a.rec_off + a.col0 + c) * caps + si];
    } else {   // lanes run along the env's row: consecutive lanes read consecutive words of it
      for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int j = idx / a.ncols, c = idx - j * a.ncols, e = s_si[j];
        if (e >= 0) s_tile[c * 65 + j] = GPTR(a.base)[(size_t)e * a.L + a.col0 + c];
      }
    }
    __syncthreads();
    if (DST_BANK) {
      for (int c = wv; c < a.ncols; c += 4)
        if (act_api) GPTR(X.bank)[(size_t)(a.rec_off + a.col0 + c) * caps + di] = s_tile[c * 65 + lane];
    } else {
      for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int j = idx / a.ncols, c = idx - j * a.ncols, e = s_di[j];
        if (e >= 0) GPTR(a.base)[(size_t)e * a.L + a.col0 + c] = s_tile[c * 65 + j];
      }
    }
    return;
  }

  // ---------------------------------------------------------------------------------------------- packed 64-bit / 8-bit API words
  if (wv != 0 || !act_api) return;
  const int off[ST_MISC_WORDS] = {X.off_rew, X.off_reset, X.off_esc, X.off_esc + 1, X.off_elen, X.off_elen + 1,
                                  X.off_masks, X.off_masks + 1, X.off_masks + 2};
  unsigned m[ST_MISC_WORDS];
  if (SRC_BANK) {
#pragma unroll
    for (int i = 0; i < ST_MISC_WORDS; i++) m[i] = GPTR(X.bank)[(size_t)off[i] * caps + si];
  } else {
    m[0] = __float_as_uint(T.rew_buf[si]);
    m[1] = T.reset_buf[si];
    const unsigned long long a = (unsigned long long)T.episode_step_count[si], b = (unsigned long long)T.episode_length[si];
    m[2] = (unsigned)a; m[3] = (unsigned)(a >> 32); m[4] = (unsigned)b; m[5] = (unsigned)(b >> 32);
    m[6] = m[7] = m[8] = 0;
    if (T.masks) {
#pragma unroll
      for (int i = 0; i < DEXSIM_NUM_MASKS; i++) m[6 + (i >> 2)] |= (unsigned)T.masks[(size_t)i * NR + si] << (8 * (i & 3));
    }
  }
  if (DST_BANK) {
#pragma unroll
    for (int i = 0; i < ST_MISC_WORDS; i++) GPTR(X.bank)[(size_t)off[i] * caps + di] = m[i];
  } else {
    T.rew_buf[di] = __uint_as_float(m[0]);
    T.reset_buf[di] = (uint8_t)m[1];
    T.episode_step_count[di] = (int64_t)((unsigned long long)m[2] | ((unsigned long long)m[3] << 32));
    T.episode_length[di] = (int64_t)((unsigned long long)m[4] | ((unsigned long long)m[5] << 32));
    if (T.masks) {
#pragma unroll
      for (int i = 0; i < DEXSIM_NUM_MASKS; i++) T.masks[(size_t)i * NR + di] = (uint8_t)(m[6 + (i >> 2)] >> (8 * (i & 3)));
    }
  }
}
