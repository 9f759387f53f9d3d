// Shared device/host helpers for the gfx950 kernels. CDNA4 only: 64-lane wavefronts are assumed throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include <type_traits>

#include "../../include/matcha_hip.h"

namespace matcha {

constexpr int kWave = 64;

void set_error(const char* fmt, ...);

#define MATCHA_CHECK_ARG(cond, ...)              \
  do {                                           \
    if (!(cond)) {                               \
      ::matcha::set_error(__VA_ARGS__);          \
      return MATCHA_EINVAL;                      \
    }                                            \
  } while (0)

// Launch log (matcha_launch_log / matcha_launch_log_read): every launch site names its kernel here, so a test can assert WHICH
// kernels an entry point ran -- a size rule must not move a parity test onto another kernel unnoticed.  Off: one branch.
extern int g_launch_log;
void note_launch(const char* name);

#define MATCHA_CHECK_LAUNCH(name)                                                       \
  do {                                                                                  \
    if (::matcha::g_launch_log) ::matcha::note_launch(name);                            \
    hipError_t e__ = hipGetLastError();                                                 \
    if (e__ != hipSuccess) {                                                            \
      ::matcha::set_error("launch of %s failed: %s", name, hipGetErrorString(e__));     \
      return MATCHA_EHIP;                                                               \
    }                                                                                   \
  } while (0)

#define MATCHA_TRY(expr)          \
  do {                            \
    int rc__ = (expr);            \
    if (rc__ != MATCHA_OK) return rc__; \
  } while (0)

// Optional per-kernel-class timing with HIP events on the launch stream (matcha_profile_select/_read):
// bench.py uses it to time the dominant kernel live, inside the timed region.  Off by default (one branch).
extern int g_prof_class;
void prof_record(bool start, double work, hipStream_t st);
struct ProfScope {
  bool on;
  hipStream_t st;
  ProfScope(int cls, double work, hipStream_t s) : on(cls == g_prof_class), st(s) { if (on) prof_record(true, work, st); }
  ~ProfScope() { if (on) prof_record(false, 0.0, st); }
};

// Compute units of the CURRENT device (hipGetDevice), cached per device id: grids and slab counts of the persistent kernels are sized from
// it, and a process may drive more than one device (the per-file function-static caches kept the first device's count).
int device_cu_count();

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Kernels templated on the hyperedge width keep register arrays of the smallest instantiated width >= L: 2, 3, 4, 5, 6 or 8.
inline int ml_of(int L) { return L <= 2 ? 2 : (L <= 6 ? L : 8); }
// ... and their launchers pick the instance through a generic lambda: f(std::integral_constant<int, ML>{})
template <class F>
inline void dispatch_ml(int L, F&& f) {
  switch (ml_of(L)) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

// ---- counter-based RNG: the specification is oracle/rng.py (bit-identical) ---------------------
__host__ __device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ uint32_t rng_key(uint64_t seed, uint32_t stream) {
  uint32_t k = lowbias32(stream + 0x9E3779B9u);
  k = lowbias32((uint32_t)(seed >> 32) ^ k);
  k = lowbias32((uint32_t)(seed & 0xFFFFFFFFu) ^ k);
  return k;
}
__host__ __device__ __forceinline__ uint32_t rng_u32(uint32_t key, uint32_t hi, uint32_t lo) {
  return lowbias32(lo ^ lowbias32(hi ^ key));
}
__host__ __device__ __forceinline__ uint32_t dropout_threshold(float p) {
  double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
}
constexpr uint32_t kStreamDropAdj = 1, kStreamDropFc1 = 2, kStreamDropPff = 3, kStreamNeg = 16, kStreamOutlier = 18,
                   kStreamWalk = 19, kStreamSgns = 20;

// ---- inverse CDF over an integer cumulative table (walk.hip, sgns.hip) -------------------------
// cum[0 .. n) is an inclusive prefix sum of positive integer weights, total = cum[n - 1].  The draw is r = floor(u * total / 2^64) for a
// 64-bit uniform u, the answer the first i with cum[i] > r: index i is drawn with probability (cum[i] - cum[i - 1]) / total up to 2^-64.
__device__ __forceinline__ uint64_t rng_u64(uint32_t key, uint32_t hi, uint32_t lo) {
  return ((uint64_t)rng_u32(key, hi, lo) << 32) | (uint64_t)rng_u32(key, hi, lo + 1u);
}
__device__ __forceinline__ int64_t cum_draw(const uint64_t* __restrict__ cum, int64_t n, uint64_t u) {
  const uint64_t r = __umul64hi(u, cum[n - 1]);
  int64_t lo = 0, hi = n - 1;                          // the answer lies in [lo, hi]: cum[n - 1] = total > r
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cum[mid] > r) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// ---- wave-level reductions over groups of 2^k adjacent lanes -----------------------------------
template <int WIDTH>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
// Sum over groups of 8 adjacent lanes with DPP cross-lane moves (VALU rate) instead of ds_bpermute shuffles (each a
// trip through the LDS crossbar): quad_perm [1,0,3,2], quad_perm [2,3,0,1], then row_half_mirror (lane i <-> 7 - i of
// each 8, which pairs the two quads).  Every lane ends with the group's total.
__device__ __forceinline__ float group_sum8_dpp(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  return v;
}
// Sum over groups of 16 adjacent lanes (one DPP row): the 8-lane tree, then row_mirror (lane i <-> 15 - i).
__device__ __forceinline__ float group_sum16_dpp(float v) {
  v = group_sum8_dpp(v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
  return v;
}

// tanh through one v_exp: (e^{2x} - 1) / (e^{2x} + 1), whose error is ~1e-7 ABSOLUTE -- relative 1e-7 / |x|, 6e-6 at |x| = 0.01 -- so
// below |x| = 0.5 the odd Taylor polynomial to x^15 takes over (truncation < 1e-8, ~1 ulp relative in f32 Horner form; measured by
// tests/test_hip_fp64_grade.py's small-amplitude cases).  libm's tanhf costs ~40 VALU instructions, which are not free next to the f32
// MFMAs (tools/ubench/mfma_valu.hip); both branches here are straight-line and the result is a select.
__device__ __forceinline__ float fast_tanh(float x) {
  const float xc = fminf(fmaxf(x, -15.f), 15.f);
  const float e = __expf(2.f * xc);
  const float big = (e - 1.f) * __builtin_amdgcn_rcpf(e + 1.f);
  const float x2 = x * x;
  float p = -1.4558344e-3f;                  // -929569/638512875
  p = fmaf(p, x2, 3.5921280e-3f);            //  21844/6081075
  p = fmaf(p, x2, -8.8632355e-3f);           // -1382/155925
  p = fmaf(p, x2, 2.1869488e-2f);            //  62/2835
  p = fmaf(p, x2, -5.3968254e-2f);           // -17/315
  p = fmaf(p, x2, 1.3333334e-1f);            //  2/15
  p = fmaf(p, x2, -3.3333334e-1f);           // -1/3
  const float small = fmaf(x * x2, p, x);
  return fabsf(x) < 0.5f ? small : big;
}

template <int WIDTH>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

}  // namespace matcha
