// Stand-alone sweep of the range-unscaled helpers of dexsim_device.h (rcp_n, div_n, sqrt_n, rsq_n) against the operators
// they replace on the step path, compiled with the library's code-generation flags (tests/test_range_unscaled_math.py).
//   unary: every one of the 2^32 bit patterns x through rcp_n / 1.f / x, sqrt_n / sqrtf, rsq_n / 1.f / sqrtf
//   div  : 2^26 seeded pairs (a, b) with a, b and a / b in [2^-60, 2^60] (both signs) through div_n / a / b
// Mismatching bit patterns (two NaNs count as equal) are counted on the device per binade = (sign, exponent field) of x (unary)
// or of the quotient (div), separately for "in range" (operand and the operator's result normal; for sqrt also x = +-0, which
// sqrt_n's precondition includes) and "outside".  Only the counts come back; they are printed one record per line:
//   <function> <sign> <exponent field> <in-range tested> <in-range mismatches> <outside tested> <outside mismatches>
#include <cstdint>
#include <cstdio>

#include "../dexrobot_isaac_amd/csrc/dexsim_device.h"

#define NBIN 512          /* sign * 256 + exponent field */
#define NFUNC 4           /* rcp sqrt rsq div */
#define NCNT 4            /* in-range tested, in-range mismatches, outside tested, outside mismatches */
#define DIV_PAIRS (1u << 26)

#define CHECK(x) do { hipError_t err_ = (x); if (err_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(err_)); return 2; } } while (0)

DI bool is_normal_bits(uint32_t u) { const uint32_t ex = (u >> 23) & 255u; return ex >= 1u && ex <= 254u; }
DI bool is_nan_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }

// one comparison into a thread's four counters of a function
DI void tally(unsigned (&c)[NCNT], bool in_range, float ref, float got) {
  const uint32_t r = __float_as_uint(ref), g = __float_as_uint(got);
  const bool same = r == g || (is_nan_bits(r) && is_nan_bits(g));
  c[in_range ? 0 : 2] += 1u;
  if (!same) c[in_range ? 1 : 3] += 1u;
}

// block b sweeps the 2^20 patterns b * 2^20 ..: part of one binade, so the block has one histogram bin.  One kernel per function
// F = 0 rcp, 1 sqrt, 2 rsq: a kernel that holds both sqrtf(x) and 1.f / sqrtf(x) computes the latter from the former's root, not
// as the v_rsq_f32 sequence that 1.f / sqrtf(x) is on its own.
template <int F>
__global__ void __launch_bounds__(256) k_unary(unsigned* __restrict__ cnt) {
  __shared__ unsigned s_cnt[NCNT];
  if (threadIdx.x < NCNT) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t base = blockIdx.x << 20, bin = base >> 23;   // grid = 4096 blocks; bin < 512
  unsigned c[NCNT] = {};
  for (uint32_t i = threadIdx.x; i < (1u << 20); i += 256u) {
    const uint32_t u = base + i;
    const float x = __uint_as_float(u);
    const bool xn = is_normal_bits(u), xz = (u & 0x7fffffffu) == 0u;
    const float ref = F == 0 ? 1.f / x : (F == 1 ? sqrtf(x) : 1.f / sqrtf(x));
    const float got = F == 0 ? rcp_n(x) : (F == 1 ? sqrt_n(x) : rsq_n(x));
    tally(c, (xn && is_normal_bits(__float_as_uint(ref))) || (F == 1 && xz), ref, got);
  }
#pragma unroll
  for (int w = 0; w < NCNT; w++) atomicAdd(&s_cnt[w], c[w]);
  __syncthreads();
  if (threadIdx.x < NCNT) atomicAdd(cnt + ((size_t)F * NBIN + bin) * NCNT + threadIdx.x, s_cnt[threadIdx.x]);
}

// a float of the given sign with a random mantissa and the unbiased exponent ex in [-60, 59]: |value| in [2^-60, 2^60)
DI float make_float(uint32_t sign, int ex, uint32_t mant23) { return __uint_as_float((sign << 31) | ((uint32_t)(ex + 127) << 23) | mant23); }

__global__ void __launch_bounds__(256) k_div(unsigned* __restrict__ cnt, unsigned* __restrict__ out_of_sample, uint32_t seed) {
  __shared__ unsigned s_cnt[NBIN * NCNT];
  for (int i = threadIdx.x; i < NBIN * NCNT; i += 256) s_cnt[i] = 0u;
  __syncthreads();
  const uint32_t stride = gridDim.x * 256u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < DIV_PAIRS; i += stride) {
    uint32_t rnd[4];
    philox4x32(rnd, i, 0u, 0u, 0u, seed, 0x5eedu);
    // exponent of b anywhere in [-60, 59]; exponent of a so that 2^-59 <= 2^(ea - eb) <= 2^59: the quotient of two values with
    // mantissas in [1, 2) is within a factor 2 of that, i.e. inside [2^-60, 2^60]
    const int eb = (int)(rnd[2] % 120u) - 60;
    const int lo = max(-60, eb - 59), hi = min(59, eb + 59);
    const int ea = lo + (int)((rnd[2] >> 8) % (uint32_t)(hi - lo + 1));
    const float a = make_float(rnd[3] & 1u, ea, rnd[0] >> 9), b = make_float((rnd[3] >> 1) & 1u, eb, rnd[1] >> 9);
    const float ref = a / b, got = div_n(a, b);
    const float m = fabsf(ref);
    if (!(m >= 0x1p-60f && m <= 0x1p60f)) { atomicAdd(out_of_sample, 1u); continue; }   // (never: see above)
    const uint32_t r = __float_as_uint(ref), g = __float_as_uint(got), bin = r >> 23;   // bin < 512
    atomicAdd(&s_cnt[bin * NCNT], 1u);
    if (r != g) atomicAdd(&s_cnt[bin * NCNT + 1], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NBIN * NCNT; i += 256)
    if (s_cnt[i]) atomicAdd(cnt + (size_t)3 * NBIN * NCNT + i, s_cnt[i]);
}

int main() {
  static unsigned h_cnt[NFUNC * NBIN * NCNT];
  unsigned *d_cnt = nullptr, *d_oos = nullptr, h_oos = 0;
  CHECK(hipMalloc(&d_cnt, sizeof(h_cnt)));
  CHECK(hipMalloc(&d_oos, sizeof(unsigned)));
  CHECK(hipMemset(d_cnt, 0, sizeof(h_cnt)));
  CHECK(hipMemset(d_oos, 0, sizeof(unsigned)));
  k_unary<0><<<dim3(4096), dim3(256)>>>(d_cnt);
  CHECK(hipGetLastError());
  k_unary<1><<<dim3(4096), dim3(256)>>>(d_cnt);
  CHECK(hipGetLastError());
  k_unary<2><<<dim3(4096), dim3(256)>>>(d_cnt);
  CHECK(hipGetLastError());
  k_div<<<dim3(1024), dim3(256)>>>(d_cnt, d_oos, 20240607u);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(&h_oos, d_oos, sizeof(unsigned), hipMemcpyDeviceToHost));
  static const char* names[NFUNC] = {"rcp", "sqrt", "rsq", "div"};
  for (int f = 0; f < NFUNC; f++)
    for (int b = 0; b < NBIN; b++) {
      const unsigned* c = h_cnt + ((size_t)f * NBIN + b) * NCNT;
      if (c[0] | c[2]) printf("%s %d %d %u %u %u %u\n", names[f], b >> 8, b & 255, c[0], c[1], c[2], c[3]);
    }
  printf("div_out_of_sample %u\n", h_oos);
  CHECK(hipFree(d_cnt));
  CHECK(hipFree(d_oos));
  return 0;
}
