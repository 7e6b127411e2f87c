// BatchNorm1d (+ReLU) over the active voxels: modules/model/sparse_unet3d.py:128-137,
// modules/model/backbone_3D_WSIS.py:47,52-55.  The reference runs BN and ReLU as separate torch ops
// (several elementwise passes + atomics-free but multi-kernel reductions); here
//   forward  = stats (one read of x, fixed-order tree)  + apply(+ReLU) (one read, one write)
//   backward = reduce (dgamma, dbeta; reads x, dy)      + apply (reads x, dy; writes dx)
// All reductions use per-workgroup partials combined in a fixed order (Chan's formula for mean/M2), so the
// result is run-to-run deterministic.  HBM-bound: 2*M*C*4 bytes per pass.
//
// Layout of this file: the arithmetic of one element, of one statistics finish and of one chunk of partial rows is
// defined ONCE (bn_fwd_elem, bn_bwd_elem, bn_bwd_dx, bn_shifted_mean_var, common.h bn_centred_mean_var / bn_store_stats,
// bn_chunk_walk / bn_lane_fold / bn_ticket_sum); every launch form -- stand-alone two-launch and one-launch, two-level
// from centred partials, small finish + apply, polled finish + apply (EXPERIMENTAL) -- is a walk around those, so the
// forms agree bit for bit by construction.  The stand-alone reductions and the backward apply are templates on the element
// type: the 16-bit entry points (wsis_bn_stats_lp, wsis_bn_bwd_lp, wsis_bn_bwd_apply_lp, wsis_bn_apply_lp) are the fp32
// kernels reading bf16 / fp16 rows widened exactly, with the fp32 forms' launch plans (bn_stats_run, bn_bwd_reduce_run).
// The wsis_bn_sync_* helpers of a layer whose statistics are shared across ranks stand at the end of the namespace.
#include <cstdlib>
#include <initializer_list>

#include "common.h"

using namespace wsis;

namespace {

constexpr int BN_ROWS_PER_THREAD = 8;   // rows one thread accumulates: all 8 (x, dy) loads are in flight at once
// rows reduced by one workgroup: 256 threads = G channel groups x R row lanes, 8 rows per lane.  (A fixed 256 rows
// made a thread of the wide levels walk 26-32 rows four at a time: 7-8 memory latencies per launch.)
__host__ __device__ inline int bn_rows_per_wg(int Cp) {
  const int G = Cp >> 2;
  const int R = 256 / G > 1 ? 256 / G : 1;
  return R * BN_ROWS_PER_THREAD;
}
constexpr int BN_THREADS = 256;

struct f4 {
  float v[4];
};
// four consecutive elements of an fp32 / bf16 / fp16 tensor as fp32 (16-bit values widen exactly), and back: float4 moves
// 16 bytes, a 16-bit quad 8 bytes (one ushort4); 16-bit stores round to nearest even
template <typename T>
__device__ __forceinline__ float4 bn_ld4(const T* p, int64_t t) {
  if constexpr (sizeof(T) == 4) {
    return reinterpret_cast<const float4*>(p)[t];
  } else {
    const ushort4 u = reinterpret_cast<const ushort4*>(p)[t];
    return make_float4((float)__builtin_bit_cast(T, u.x), (float)__builtin_bit_cast(T, u.y),
                       (float)__builtin_bit_cast(T, u.z), (float)__builtin_bit_cast(T, u.w));
  }
}
template <typename T>
__device__ __forceinline__ void bn_st4(T* p, int64_t t, float4 v) {
  if constexpr (sizeof(T) == 4) {
    reinterpret_cast<float4*>(p)[t] = v;
  } else {
    ushort4 u;
    u.x = __builtin_bit_cast(unsigned short, (T)v.x);
    u.y = __builtin_bit_cast(unsigned short, (T)v.y);
    u.z = __builtin_bit_cast(unsigned short, (T)v.z);
    u.w = __builtin_bit_cast(unsigned short, (T)v.w);
    reinterpret_cast<ushort4*>(p)[t] = u;
  }
}

// four channels of a row as fp32 (T = float, __bf16 or _Float16): one bn_ld4 quad where the row allows it.  The reductions
// and the backward apply below are written once for the three element types.
template <typename T>
__device__ __forceinline__ f4 ld4(const T* p, bool vec) {
  f4 r;
  if (vec) {
    const float4 t = bn_ld4(p, 0);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = (float)p[0]; r.v[1] = (float)p[1]; r.v[2] = (float)p[2]; r.v[3] = (float)p[3];
  }
  return r;
}

// ---- one element

// forward: fma(x - mean, sc, beta) with sc = gamma * rsqrt(var + eps): x - mean first (x*sc + (beta - mean*sc) cancels
// when |mean| >> sigma), one rounding for the scale-and-shift; the convolutions that apply the BatchNorm while they read
// their input (csrc/spconv2.hip bnfrag, csrc/spconv_dw2.hip) use the same expression, so fused and unfused passes agree
// bit for bit
__device__ __forceinline__ float bn_fwd_coef(float gamma, float var, float eps) { return gamma * rsqrtf(var + eps); }
__device__ __forceinline__ float bn_fwd_elem(float x, float mu, float sc, float bt, int relu) {
  float z = __builtin_fmaf(x - mu, sc, bt);
  if (relu) z = fmaxf(z, 0.0f);
  return z;
}

// backward: per-channel coefficients of (up to) four channels, the ReLU-masked gradient dz with the normalised input xh,
// and dx = gamma*rstd*(dz - dbeta/M - xhat*dgamma/M) (training); gamma*rstd*dz (eval), plus the addend if there is one
struct BnBwdCoef {
  float mu[4], rstd[4], gm[4], bt[4];
  __device__ __forceinline__ void load(int e, int c, const float* __restrict__ mean, const float* __restrict__ var,
                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps) {
    mu[e] = mean[c];
    rstd[e] = rsqrtf(var[c] + eps);
    gm[e] = gamma ? gamma[c] : 1.0f;
    bt[e] = beta ? beta[c] : 0.0f;
  }
};
struct BnDz {
  float dz, xh;
};
__device__ __forceinline__ BnDz bn_bwd_elem(float x, float dy, const BnBwdCoef& k, int e, int relu) {
  const float xh = (x - k.mu[e]) * k.rstd[e];
  float dz = dy;
  if (relu && xh * k.gm[e] + k.bt[e] <= 0.0f) dz = 0.0f;
  return {dz, xh};
}
__device__ __forceinline__ float bn_bwd_dx(BnDz z, const BnBwdCoef& k, int e, float k1, float k2, int training,
                                           bool has_addend, float addend) {
  float r = z.dz;
  if (training) r = z.dz - k1 - z.xh * k2;
  float o = k.gm[e] * k.rstd[e] * r;
  if (has_addend) o += addend;
  return o;
}

// ---- stand-alone reductions over x (and dy)

// Thread layout of the reductions: channels are handled in groups of 4 (one 16-byte load per row);
// 256 threads = G channel groups x R row lanes.  C is padded to C4*4 logically; tail channels are masked.
// pivot of channel c: the mean of its first (up to) 8 rows, fp32, fixed order.  Every sum of the statistics pass is
// taken of x - K: fp32 sums of the raw x and x^2 cancel in var = E[x^2] - mean^2 when |mean| >> sigma (|mean| = 1000
// sigma: 10 % off); a pivot within sigma / sqrt(8) of the mean keeps sum (x - K)^2 within 12 % of the centred sum (a
// one-row pivot doubles it, and with it the rounding error: median gradient error against the fp64 oracle 3.7e-4 ->
// 6.6e-4)
template <typename T>
__device__ __forceinline__ float bn_pivot(const T* __restrict__ x, int64_t M, int C, int c) {
  const int n = M < 8 ? (int)M : 8;
  float s = 0.0f;
  for (int r = 0; r < n; ++r) s += (float)x[(int64_t)r * C + c];
  return s / (float)n;
}

// mean / var from the fp64 sums S, Q of x - K and (x - K)^2
__device__ __forceinline__ BnMeanVar bn_shifted_mean_var(double S, double Q, float K, int64_t M) {
  const double n = (double)M;
  const double ms = S / n;              // mean of x - K
  const double mu = (double)K + ms;
  double v = Q / n - ms * ms;
  if (v < 0.0) v = 0.0;
  return {mu, v};
}

// What row r contributes to the two fp32 sums (sa, sb) of a thread that owns channels c .. c + 3: init() loads the
// per-channel values once, row() adds one row.  T: element type of x (and dy): float, or __bf16 / _Float16 widened as
// they are read -- the sums of a 16-bit tensor are the sums of the widened tensor, addition for addition.
template <typename T>
struct BnStatsAcc {      // forward: (sum, sum of squares) of x - K
  const T* __restrict__ x;
  float K[4];
  __device__ __forceinline__ void init(int64_t M, int C, int c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) K[e] = (c + e < C) ? bn_pivot(x, M, C, c + e) : 0.0f;
  }
  __device__ __forceinline__ void row(int64_t r, int C, int c, bool vec, float (&sa)[4], float (&sb)[4]) const {
    float v[4];
    if (vec) {
      const f4 t = ld4(x + r * C + c, true);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = t.v[e] - K[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (c + e < C) ? (float)x[r * C + c + e] - K[e] : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sa[e] += v[e];
      sb[e] += v[e] * v[e];
    }
  }
};
template <typename T>
struct BnBwdAcc {        // backward: (sum dz, sum dz * xhat)
  const T* __restrict__ x;
  const T* __restrict__ dy;
  const float* __restrict__ mean;
  const float* __restrict__ var;
  const float* __restrict__ gamma;
  const float* __restrict__ beta;
  float eps;
  int relu;
  BnBwdCoef k;
  __device__ __forceinline__ void init(int64_t M, int C, int c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) k.load(e, min(c + e, C - 1), mean, var, gamma, beta, eps);
  }
  __device__ __forceinline__ void row(int64_t r, int C, int c, bool vec, float (&sa)[4], float (&sb)[4]) const {
    float xv[4], dv[4];
    if (vec) {
      const f4 tx = ld4(x + r * C + c, true), td = ld4(dy + r * C + c, true);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xv[e] = tx.v[e];
        dv[e] = td.v[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = c + e < C;
        xv[e] = ok ? (float)x[r * C + c + e] : 0.0f;
        dv[e] = ok ? (float)dy[r * C + c + e] : 0.0f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const BnDz z = bn_bwd_elem(xv[e], dv[e], k, e, relu);
      sa[e] += z.dz;
      sb[e] += z.dz * z.xh;
    }
  }
};

// pass 1: per-workgroup sums per channel from ONE read of the rows.  partial [nblk][2][Cp].  s_a, s_b: BN_THREADS * 4
// floats of LDS each.
template <class Acc>
__device__ __forceinline__ void bn_partial_body(Acc acc, int64_t M, int C, int Cp, float* __restrict__ partial,
                                                float* s_a, float* s_b) {
  const int G = Cp >> 2;                       // channel groups
  const int R = max(BN_THREADS / G, 1);        // row lanes
  const bool vec = (C & 3) == 0;
  const int64_t r0 = (int64_t)blockIdx.x * bn_rows_per_wg(Cp);
  const int64_t r1 = min(M, r0 + bn_rows_per_wg(Cp));
  for (int g0 = 0; g0 < G; g0 += BN_THREADS) {  // G <= 256 in practice: one trip
    // (the divisor is spelled out at both divisions: the compiler then sees a divisor of at most 256 under a dividend
    // below 256 and emits the short reciprocal form instead of the general 32-bit one)
    const int g = g0 + (threadIdx.x % min(G, BN_THREADS));
    const int rl = threadIdx.x / min(G, BN_THREADS);
    float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
    if (g < G && rl < R) {
      const int c = g * 4;
      acc.init(M, C, c);
#pragma unroll 8
      for (int64_t r = r0 + rl; r < r1; r += R) acc.row(r, C, c, vec, sa, sb);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s_a[threadIdx.x * 4 + e] = sa[e];
      s_b[threadIdx.x * 4 + e] = sb[e];
    }
    __syncthreads();
    if (g < G && rl == 0) {
      const int gw = min(G, BN_THREADS);
      float ta[4] = {0.f, 0.f, 0.f, 0.f}, tb[4] = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < R; ++j)   // fixed order
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ta[e] += s_a[(j * gw + (threadIdx.x % gw)) * 4 + e];
          tb[e] += s_b[(j * gw + (threadIdx.x % gw)) * 4 + e];
        }
      float* p = partial + (int64_t)blockIdx.x * 2 * Cp;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[g * 4 + e] = ta[e];
        p[Cp + g * 4 + e] = tb[e];
      }
    }
    __syncthreads();
  }
}

// forward: partial sums of x - K and (x - K)^2
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_partial_kernel(const T* __restrict__ x, int64_t M, int C, int Cp,
                                                                      float* __restrict__ partial) {
  __shared__ float s_a[BN_THREADS * 4];
  __shared__ float s_b[BN_THREADS * 4];
  bn_partial_body(BnStatsAcc<T>{x}, M, C, Cp, partial, s_a, s_b);
}

// backward pass 1: per-workgroup partial (sum dz, sum dz*xhat) per channel
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_partial_kernel(
    const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    int relu, int64_t M, int C, int Cp, float* __restrict__ partial) {
  __shared__ float s_a[BN_THREADS * 4];
  __shared__ float s_b[BN_THREADS * 4];
  bn_partial_body(BnBwdAcc<T>{x, dy, mean, var, gamma, beta, eps, relu}, M, C, Cp, partial, s_a, s_b);
}

// pass 2: one wavefront per channel: lanes stride over the partials (fp64), fixed butterfly => deterministic.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ void bn_final_sums(const float* __restrict__ partial, int nblk, int Cp, int c, double& A,
                                              double& B) {
  double a = 0.0, b = 0.0;
#pragma unroll 8
  for (int k = threadIdx.x; k < nblk; k += 64) {
    a += partial[(int64_t)k * 2 * Cp + c];
    b += partial[(int64_t)k * 2 * Cp + Cp + c];
  }
  A = wave_sum_f64(a);
  B = wave_sum_f64(b);
}

template <typename T>
__global__ __launch_bounds__(64) void bn_stats_final_kernel(const float* __restrict__ partial, int nblk, int C,
                                                            int Cp, int64_t M, const T* __restrict__ x0,
                                                            float* __restrict__ mean,
                                                            float* __restrict__ var,
                                                            float* __restrict__ running_mean,
                                                            float* __restrict__ running_var, float momentum) {
  const int c = blockIdx.x;
  double S, Q;
  bn_final_sums(partial, nblk, Cp, c, S, Q);
  if (threadIdx.x == 0)
    bn_store_stats(bn_shifted_mean_var(S, Q, bn_pivot(x0, M, C, c), M), M, c, mean, var, running_mean, running_var,
                   momentum);
}

__global__ __launch_bounds__(64) void bn_bwd_final_kernel(const float* __restrict__ partial, int nblk, int C, int Cp,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x;
  double A, B;
  bn_final_sums(partial, nblk, Cp, c, A, B);
  if (threadIdx.x == 0) {
    dbeta[c] = (float)A;
    dgamma[c] = (float)B;
  }
}

// ---- small inputs (M <= bn_small_rows): the whole reduction in ONE launch, one workgroup per channel group of 4.
// Two launches (partial + final) of a few microseconds each are pure latency at the deep UNet levels (<= 4096 rows;
// above that the 16-byte-per-row slices of one workgroup per channel group stall on cache-line throughput).
// 1024 threads stride over the rows (<= 8 rows each, every load in flight at once: the kernel is one memory latency
// long, not M/256 of them), then a fixed reduction in fp64: xor-shuffle inside each wave, 16 wave results through
// LDS, summed in wave order -> deterministic.
int64_t bn_small_rows() {  // WSIS_BN_SMALL_ROWS: rows up to which the one-launch reduction is used
  static const int64_t v = [] {
    const char* e = getenv("WSIS_BN_SMALL_ROWS");
    return e ? (int64_t)atoll(e) : (int64_t)4096;
  }();
  return v;
}
constexpr int BN_SMALL_THREADS = 1024;

__device__ __forceinline__ void block_sum2_f64(double (&a)[4], double (&b)[4], double* sh) {
  // sh: [BN_SMALL_THREADS / 64][8] doubles
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] += __shfl_xor(a[e], off, 64);
      b[e] += __shfl_xor(b[e], off, 64);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sh[wave * 8 + e] = a[e];
      sh[wave * 8 + 4 + e] = b[e];
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double sa = 0.0, sb = 0.0;
    for (int w = 0; w < BN_SMALL_THREADS / 64; ++w) {
      sa += sh[w * 8 + e];
      sb += sh[w * 8 + 4 + e];
    }
    a[e] = sa;
    b[e] = sb;
  }
}

// the sums of channels c0 .. c0 + 3 over all M rows, in every thread: a[e], b[e]
template <class Acc>
__device__ __forceinline__ void bn_small_body(Acc& acc, int64_t M, int C, int c0, double* sh, double (&a)[4],
                                              double (&b)[4]) {
  const bool vec = (C & 3) == 0;
  acc.init(M, C, c0);
  float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int64_t r = threadIdx.x; r < M; r += BN_SMALL_THREADS) acc.row(r, C, c0, vec, sa, sb);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = sa[e];
    b[e] = sb[e];
  }
  block_sum2_f64(a, b, sh);
}

template <typename T>
__global__ __launch_bounds__(BN_SMALL_THREADS) void bn_stats_small_kernel(const T* __restrict__ x, int64_t M, int C,
                                                                    float* __restrict__ mean, float* __restrict__ var,
                                                                    float* __restrict__ running_mean,
                                                                    float* __restrict__ running_var, float momentum) {
  __shared__ double sh[BN_SMALL_THREADS / 64 * 8];
  const int c0 = blockIdx.x * 4;
  BnStatsAcc<T> acc{x};
  double a[4], b[4];
  bn_small_body(acc, M, C, c0, sh, a, b);
  const float K[4] = {acc.K[0], acc.K[1], acc.K[2], acc.K[3]};      // (indexed by the thread: an array of its own)
  if (threadIdx.x < 4 && c0 + (int)threadIdx.x < C) {
    const int e = threadIdx.x;
    bn_store_stats(bn_shifted_mean_var(a[e], b[e], K[e], M), M, c0 + e, mean, var, running_mean, running_var, momentum);
  }
}

template <typename T>
__global__ __launch_bounds__(BN_SMALL_THREADS) void bn_bwd_small_kernel(
    const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    int relu, int64_t M, int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double sh[BN_SMALL_THREADS / 64 * 8];
  const int c0 = blockIdx.x * 4;
  BnBwdAcc<T> acc{x, dy, mean, var, gamma, beta, eps, relu};
  double a[4], b[4];
  bn_small_body(acc, M, C, c0, sh, a, b);
  if (threadIdx.x < 4 && c0 + (int)threadIdx.x < C) {
    dbeta[c0 + threadIdx.x] = (float)a[threadIdx.x];
    dgamma[c0 + threadIdx.x] = (float)b[threadIdx.x];
  }
}

// ---- two-level reductions of per-slice partials [nblk][2][C], written by the convolution epilogues (csrc/spconv2.hip).
// Forward (NT = 3 totals S, Q, W): slice i holds S_i = sum and Q_i = sum of squared deviations from ITS mean over
// n_i = min(32, M - 32 i) rows; mean = sum S_i / M, var = (sum Q_i + sum S_i^2 / n_i - M mean^2) / M, all in fp64 (Chan's
// pairwise combination).  Backward (NT = 2 totals dbeta, dgamma): slice i holds (sum dz, sum dz * xhat), written by the
// epilogue of the dIn convolution that produced dy (wsis_spconv_fwd_t_bn).
// Two levels so that the 1.2 MB of partials of a 150k-row level is read by up to 64 workgroups per 32 channels instead of
// one: chunk sums (fixed order inside a chunk) -> [G][NT][C] doubles, then one thread per channel adds the chunks in order.
// Arrival tickets: one counter per channel group in the caller's sync slot (common.h SyncSlot; zero between launches:
// the last workgroup resets its counter).
constexpr int BN_FIN_CHUNKS = kBnFinChunks;      // <= 64: the finish kernels hold one chunk per lane

// 256 threads = 32 channel lanes (cl) x 8 partial lanes (pl).  Lane pl of channel c adds rows lo + pl, + 8, ... < hi of the
// partials to t; the forward totals also take W += S_i^2 / n_i.
template <int NT>
__device__ __forceinline__ void bn_chunk_walk(const float* __restrict__ partial, int lo, int hi, int C, int64_t M, int c,
                                              double (&t)[NT]) {
  const int pl = threadIdx.x >> 5;
  if (c < C) {
#pragma unroll 4
    for (int b = lo + pl; b < hi; b += 8) {
      const float sf = partial[(int64_t)b * 2 * C + c];
      const float qf = partial[(int64_t)b * 2 * C + C + c];
      const double si = sf;
      t[0] += si;
      t[1] += qf;
      if constexpr (NT == 3) {
        const int64_t left = M - (int64_t)b * 32;
        t[2] += si * si * (left < 32 ? 1.0 / (double)left : 0.03125);
      }
    }
  }
}
// the 8 lane sums of a channel through LDS, added in lane order (fixed order): T, in the threads with `own` (pl == 0 and
// a channel below C)
template <int NT>
__device__ __forceinline__ void bn_lane_fold(const double (&t)[NT], bool own, double (&red)[NT][8][33], double (&T)[NT]) {
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < NT; ++k) red[k][pl][cl] = t[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NT; ++k) T[k] = 0.0;
  if (own) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int k = 0; k < NT; ++k) T[k] += red[k][j][cl];
  }
}
__device__ __forceinline__ void bn_chunk_range(int nblk, int G, int g, int& lo, int& hi) {
  const int per = (nblk + G - 1) / G;
  lo = g * per;
  hi = lo + per < nblk ? lo + per : nblk;
}

// Chunk g0 of G > 1 hands its totals T to the workgroup that arrives last (per channel group), which adds the chunks,
// always in chunk order: one launch instead of two.  The chunk rows cross XCDs as sc1 stores / sc1 loads around the
// ticket (common.h): no fences, each of which costs more than the rest of this stage.  Returns true in that last workgroup,
// with the totals of all chunks in T (threads with `own`); without tickets a second launch adds the chunks.
template <int NT>
__device__ __forceinline__ bool bn_ticket_sum(double* __restrict__ chunk, unsigned* __restrict__ ticket, int g0, int G,
                                              int cgi, int C, int c, bool own, double (&T)[NT],
                                              double (&red)[NT][8][33], int& s_last) {
  if (own) {
    double* o = chunk + (int64_t)g0 * NT * C;
#pragma unroll
    for (int k = 0; k < NT; ++k) st_sc1(o + k * C + c, T[k]);
  }
  if (!ticket) return false;
  wait_stores_left();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = atomicAdd(ticket + cgi, 1u);
    s_last = t == (unsigned)G - 1;
    if (s_last) ticket[cgi] = 0u;          // self-cleaning: ready for the next launch on this stream
  }
  __syncthreads();
  if (!s_last) return false;
  double t2[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) t2[k] = 0.0;
  if (c < C)
    for (int g = threadIdx.x >> 5; g < G; g += 8) {
      const double* o = chunk + (int64_t)g * NT * C;
#pragma unroll
      for (int k = 0; k < NT; ++k) t2[k] += ld_sc1(o + k * C + c);
    }
  __syncthreads();            // `red` of the chunk's own fold has been read by everyone
  bn_lane_fold<NT>(t2, own, red, T);
  return true;
}

// chunk g0 of G for channel group cgi; G == 1 finishes in place.  finish(c, T) writes the result of channel c from its
// totals.  Returns true in the workgroup that wrote the result of the channel group (G == 1, or the last arrival).
template <int NT, class Finish>
__device__ __forceinline__ bool bn_chunk_stage(const float* __restrict__ partial, int nblk, int C, int64_t M,
                                               double* __restrict__ chunk, unsigned* __restrict__ ticket, int g0, int G,
                                               int cgi, double (&red)[NT][8][33], int& s_last, Finish finish) {
  const int c = cgi * 32 + (threadIdx.x & 31);
  const bool own = (threadIdx.x >> 5) == 0 && c < C;
  int lo, hi;
  bn_chunk_range(nblk, G, g0, lo, hi);
  double t[NT], T[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) t[k] = 0.0;
  bn_chunk_walk<NT>(partial, lo, hi, C, M, c, t);
  bn_lane_fold<NT>(t, own, red, T);
  if (G > 1 && !bn_ticket_sum<NT>(chunk, ticket, g0, G, cgi, C, c, own, T, red, s_last)) return false;
  if (own) finish(c, T);
  return true;
}

__device__ __forceinline__ bool bn_chunk_centred_stage(const float* __restrict__ partial, int nblk, int C, int64_t M,
                                                       double* __restrict__ chunk, float* __restrict__ mean,
                                                       float* __restrict__ var, float* __restrict__ running_mean,
                                                       float* __restrict__ running_var, float momentum,
                                                       unsigned* __restrict__ ticket, int g0, int G, int cgi,
                                                       double (&red)[3][8][33], int& s_last) {
  return bn_chunk_stage<3>(partial, nblk, C, M, chunk, ticket, g0, G, cgi, red, s_last, [&](int c, const double (&T)[3]) {
    bn_finish_centred(T[0], T[1], T[2], M, c, mean, var, running_mean, running_var, momentum);
  });
}
__device__ __forceinline__ bool bn_sum_chunk_stage(const float* __restrict__ partial, int nblk, int C,
                                                   double* __restrict__ chunk, float* dbeta, float* dgamma,
                                                   unsigned* __restrict__ ticket, int g0, int G, int cgi,
                                                   double (&red)[2][8][33], int& s_last) {
  return bn_chunk_stage<2>(partial, nblk, C, 0, chunk, ticket, g0, G, cgi, red, s_last, [&](int c, const double (&T)[2]) {
    dbeta[c] = (float)T[0];
    dgamma[c] = (float)T[1];
  });
}

// grid (G, ceil(C / 32))
__global__ __launch_bounds__(256) void bn_stats_chunk_centred_kernel(const float* __restrict__ partial, int nblk, int C,
                                                                     int64_t M, double* __restrict__ chunk,
                                                                     float* __restrict__ mean, float* __restrict__ var,
                                                                     float* __restrict__ running_mean,
                                                                     float* __restrict__ running_var, float momentum,
                                                                     unsigned* __restrict__ ticket) {
  __shared__ double red[3][8][33];
  __shared__ int s_last;
  bn_chunk_centred_stage(partial, nblk, C, M, chunk, mean, var, running_mean, running_var, momentum, ticket,
                         (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.y, red, s_last);
}
__global__ __launch_bounds__(256) void bn_sum_chunk_kernel(const float* __restrict__ partial, int nblk, int C,
                                                           double* __restrict__ chunk, float* __restrict__ dbeta,
                                                           float* __restrict__ dgamma, unsigned* __restrict__ ticket) {
  __shared__ double red[2][8][33];
  __shared__ int s_last;
  bn_sum_chunk_stage(partial, nblk, C, chunk, dbeta, dgamma, ticket, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.y, red,
                     s_last);
}

// the second launch without tickets.  One wavefront per channel: lane g holds chunk g (G <= 64), fixed butterfly
__global__ __launch_bounds__(256) void bn_stats_final_centred_kernel(const double* __restrict__ chunk, int G, int C,
                                                                     int64_t M, float* __restrict__ mean,
                                                                     float* __restrict__ var,
                                                                     float* __restrict__ running_mean,
                                                                     float* __restrict__ running_var, float momentum) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const bool in = lane < G;
  const double S = wave_sum_f64(in ? chunk[(int64_t)lane * 3 * C + c] : 0.0);
  const double Q = wave_sum_f64(in ? chunk[(int64_t)lane * 3 * C + C + c] : 0.0);
  const double W = wave_sum_f64(in ? chunk[(int64_t)lane * 3 * C + 2 * C + c] : 0.0);
  if (lane == 0) bn_finish_centred(S, Q, W, M, c, mean, var, running_mean, running_var, momentum);
}
__global__ __launch_bounds__(256) void bn_sum_final_kernel(const double* __restrict__ chunk, int G, int C,
                                                           float* __restrict__ dbeta, float* __restrict__ dgamma) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const bool in = lane < G;
  const double A = wave_sum_f64(in ? chunk[(int64_t)lane * 2 * C + c] : 0.0);
  const double B = wave_sum_f64(in ? chunk[(int64_t)lane * 2 * C + C + c] : 0.0);
  if (lane == 0) {
    dbeta[c] = (float)A;
    dgamma[c] = (float)B;
  }
}

// ---- apply passes

// COHERENT: the statistics were written by other workgroups of THIS launch (the polled form below): they are read with
// agent-scope loads, which do not hit stale lines of this XCD's L2 -- cheaper than an acquire fence, whose L2 invalidate
// is serialised over the waiting workgroups of an XCD (measured: + 50 ns per waiting workgroup)
template <bool COHERENT>
__device__ __forceinline__ float bn_ld_stat(const float* p) {
  if (COHERENT) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

// TI / TO: element types of x and y (float, __bf16 or _Float16).  The arithmetic is fp32 whatever they are: a 16-bit x is
// widened exactly, y is rounded once at the store -- the 16-bit forms equal the fp32 form on the widened x, rounded.
template <bool COHERENT, typename TI = float, typename TO = float>
__device__ __forceinline__ void bn_apply_body(const TI* __restrict__ x, const float* mean,
                                              const float* var, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float eps, int relu,
                                              TO* __restrict__ y, int64_t M, int C) {
  const int64_t total = M * C;
  if ((C & 3) == 0) {
    const int64_t total4 = total >> 2;
    const unsigned C4 = (unsigned)(C >> 2);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const bool fixed_c = (stride % C4) == 0;      // then the channel group of a thread never changes
    unsigned cg = (unsigned)(t % C4);
    float sc[4], mu[4], bt[4];
    auto coef = [&](unsigned g) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = (int)g * 4 + e;
        sc[e] = bn_fwd_coef(gamma ? gamma[c] : 1.0f, bn_ld_stat<COHERENT>(var + c), eps);
        mu[e] = bn_ld_stat<COHERENT>(mean + c);
        bt[e] = beta ? beta[c] : 0.0f;
      }
    };
    coef(cg);
    auto body = [&](const float4 v) {
      float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = bn_fwd_elem(o[e], mu[e], sc[e], bt[e], relu);
      return make_float4(o[0], o[1], o[2], o[3]);
    };
    if (fixed_c) {   // two quads per trip in flight (the launcher rounds the grid so that this branch is taken)
      for (; t + stride < total4; t += 2 * stride) {
        const float4 v0 = bn_ld4(x, t);
        const float4 v1 = bn_ld4(x, t + stride);
        bn_st4(y, t, body(v0));
        bn_st4(y, t + stride, body(v1));
      }
      if (t < total4) bn_st4(y, t, body(bn_ld4(x, t)));
    } else {
      for (; t < total4; t += stride) {
        cg = (unsigned)(t % C4);
        coef(cg);
        bn_st4(y, t, body(bn_ld4(x, t)));
      }
    }
  } else {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
      const int c = (int)(t % C);
      const float sc = bn_fwd_coef(gamma ? gamma[c] : 1.0f, bn_ld_stat<COHERENT>(var + c), eps);
      y[t] = (TO)bn_fwd_elem((float)x[t], bn_ld_stat<COHERENT>(mean + c), sc, beta ? beta[c] : 0.0f, relu);
    }
  }
}

__global__ void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                const float* __restrict__ var, const float* __restrict__ gamma,
                                const float* __restrict__ beta, float eps, int relu, float* __restrict__ y,
                                int64_t M, int C) {
  bn_apply_body<false>(x, mean, var, gamma, beta, eps, relu, y, M, C);
}

// the evaluation-mode apply of a 16-bit pass (wsis_bn_apply_lp): 16-bit x, 16-bit or fp32 y
template <typename TI, typename TO>
__global__ void bn_apply_lp_kernel(const TI* __restrict__ x, const float* __restrict__ mean,
                                   const float* __restrict__ var, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float eps, int relu, TO* __restrict__ y, int64_t M,
                                   int C) {
  bn_apply_body<false, TI, TO>(x, mean, var, gamma, beta, eps, relu, y, M, C);
}

template <typename TI>
void launch_bn_apply_lp(const void* x, const float* mean, const float* var, const float* gamma, const float* beta,
                        float eps, int relu, void* y, int out_fp32, int64_t M, int C, int grid, hipStream_t st) {
  if (out_fp32)
    hipLaunchKernelGGL((bn_apply_lp_kernel<TI, float>), dim3(grid), dim3(256), 0, st, static_cast<const TI*>(x), mean,
                       var, gamma, beta, eps, relu, static_cast<float*>(y), M, C);
  else
    hipLaunchKernelGGL((bn_apply_lp_kernel<TI, TI>), dim3(grid), dim3(256), 0, st, static_cast<const TI*>(x), mean, var,
                       gamma, beta, eps, relu, static_cast<TI*>(y), M, C);
}

// backward pass 2 (bn_bwd_dx).  T: element type of x, dy and the addend, TO: of dx (T, or float for the unrounded dx of a
// 16-bit pass).  The arithmetic is fp32 whatever they are; a 16-bit dx is rounded once at the store, addend included.
template <bool COHERENT, typename T, typename TO>     // COHERENT: dgamma / dbeta come from other workgroups of this launch (see bn_ld_stat)
__device__ __forceinline__ void bn_bwd_apply_body(const T* __restrict__ x, const T* __restrict__ dy,
                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  const float* dgamma, const float* dbeta,
                                                  const T* __restrict__ addend, float eps, int relu, int training,
                                                  TO* __restrict__ dx, int64_t M, int C) {
  const int64_t total = M * C;
  const float inv_m = 1.0f / (float)M;
  const bool vec = (C & 3) == 0;
  const int W = vec ? 4 : 1;
  const int64_t totalw = total / W;
  const unsigned Cw = (unsigned)(C / W);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  // per-channel coefficients stay in registers while the thread's channel group does not change (it never does
  // when the grid stride is a multiple of the channel groups; the launcher rounds the grid to make it so)
  const bool fixed_c = (stride % Cw) == 0;
  BnBwdCoef k;
  float k1[4], k2[4];
  auto coef = [&](int c0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < W) {
        const int c = c0 + e;
        k.load(e, c, mean, var, gamma, beta, eps);
        k1[e] = training ? bn_ld_stat<COHERENT>(dbeta + c) * inv_m : 0.0f;
        k2[e] = training ? bn_ld_stat<COHERENT>(dgamma + c) * inv_m : 0.0f;
      }
    }
  };
  if (t < totalw) coef((int)(t % Cw) * W);
  auto one = [&](const float (&xv)[4], const float (&dv)[4], const float (&av)[4], float (&ov)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < W)
        ov[e] = bn_bwd_dx(bn_bwd_elem(xv[e], dv[e], k, e, relu), k, e, k1[e], k2[e], training, addend != nullptr, av[e]);
    }
  };
  if (vec && fixed_c) {   // two float4 triples per trip in flight
    for (; t + stride < totalw; t += 2 * stride) {
      const int64_t u = t + stride;
      const f4 tx0 = ld4(x + t * 4, true), td0 = ld4(dy + t * 4, true);
      const f4 tx1 = ld4(x + u * 4, true), td1 = ld4(dy + u * 4, true);
      f4 ta0, ta1;
#pragma unroll
      for (int e = 0; e < 4; ++e) ta0.v[e] = ta1.v[e] = 0.f;
      if (addend) {
        ta0 = ld4(addend + t * 4, true);
        ta1 = ld4(addend + u * 4, true);
      }
      float o0[4], o1[4];
      one(tx0.v, td0.v, ta0.v, o0);
      one(tx1.v, td1.v, ta1.v, o1);
      bn_st4(dx, t, make_float4(o0[0], o0[1], o0[2], o0[3]));
      bn_st4(dx, u, make_float4(o1[0], o1[1], o1[2], o1[3]));
    }
  }
  for (; t < totalw; t += stride) {
    if (!fixed_c) coef((int)(t % Cw) * W);
    float xv[4], dv[4], av[4] = {0.f, 0.f, 0.f, 0.f}, ov[4];
    if (vec) {
      const f4 tx = ld4(x + t * 4, true), td = ld4(dy + t * 4, true);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xv[e] = tx.v[e];
        dv[e] = td.v[e];
      }
      if (addend) {
        const f4 ta = ld4(addend + t * 4, true);
#pragma unroll
        for (int e = 0; e < 4; ++e) av[e] = ta.v[e];
      }
    } else {
      xv[0] = (float)x[t];
      dv[0] = (float)dy[t];
      if (addend) av[0] = (float)addend[t];
    }
    one(xv, dv, av, ov);
    if (vec)
      bn_st4(dx, t, make_float4(ov[0], ov[1], ov[2], ov[3]));
    else
      dx[t] = (TO)ov[0];
  }
}

template <typename T, typename TO>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                    const float* __restrict__ mean, const float* __restrict__ var,
                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                    const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                    const T* __restrict__ addend, float eps, int relu, int training,
                                    TO* __restrict__ dx, int64_t M, int C) {
  bn_bwd_apply_body<false>(x, dy, mean, var, gamma, beta, dgamma, dbeta, addend, eps, relu, training, dx, M, C);
}

// ---- levels of few chunks (rows < ~10,240): statistics finish + apply, and backward reduction finish + apply, as ONE
// launch WITHOUT any hand-off between workgroups.  Grid (row blocks, 32-channel groups); every workgroup runs the finish
// of ITS channel group itself -- the chunk sums of bn_chunk_stage, then the chunk sums added in chunk order, which is what
// the last-arriving workgroup of that stage does with one chunk per lane --, keeps the coefficients in LDS and applies
// them to its rows; row block 0 also writes mean / var / running statistics (dgamma / dbeta).  The finish launch it
// replaces is 4-5 us + a kernel boundary for a few hundred floats of work.  Same values as the two launches, bit for bit.
constexpr int BN_SF_ROWS = 256;      // rows per workgroup (32 rows x 8 float4 lanes per pass)

// totals of channel c over all G chunks, in the threads with `own`
template <int NT>
__device__ __forceinline__ void bn_small_totals(const float* __restrict__ partial, int nblk, int C, int64_t M, int G, int c,
                                                bool own, double (&red)[NT][8][33], double (&T)[NT]) {
#pragma unroll
  for (int k = 0; k < NT; ++k) T[k] = 0.0;
  for (int g = 0; g < G; ++g) {
    int lo, hi;
    bn_chunk_range(nblk, G, g, lo, hi);
    double t[NT], Tg[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k] = 0.0;
    bn_chunk_walk<NT>(partial, lo, hi, C, M, c, t);
    if (g) __syncthreads();            // (the previous chunk's lane sums have been read)
    bn_lane_fold<NT>(t, own, red, Tg);
    if (own) {
      // one chunk IS the result; several are added as 0.0 + chunk 0 + chunk 1 + ... (the order of the stage's second
      // level).  The two differ in a bit: 0.0 + (-0.0) is +0.0
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        if (G == 1)
          T[k] = Tg[k];
        else
          T[k] += Tg[k];
      }
    }
  }
}

__global__ __launch_bounds__(256) void bn_small_finish_apply_kernel(
    const float* __restrict__ partial, int nblk, int C, int64_t M, float* __restrict__ mean, float* __restrict__ var,
    float* __restrict__ running_mean, float* __restrict__ running_var, float momentum, const float* __restrict__ x,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu, float* __restrict__ y, int G) {
  __shared__ double red[3][8][33];
  __shared__ float s_mu[32], s_sc[32], s_bt[32];
  const int cgi = blockIdx.y;
  const int cl = threadIdx.x & 31;
  const int c = cgi * 32 + cl;
  const bool own = (threadIdx.x >> 5) == 0 && c < C;
  double T[3];
  bn_small_totals<3>(partial, nblk, C, M, G, c, own, red, T);
  if (own) {
    const BnMeanVar s = bn_centred_mean_var(T[0], T[1], T[2], M);
    if (blockIdx.x == 0) bn_store_stats(s, M, c, mean, var, running_mean, running_var, momentum);
    s_mu[cl] = (float)s.mu;
    s_sc[cl] = bn_fwd_coef(gamma ? gamma[c] : 1.0f, (float)s.v, eps);
    s_bt[cl] = beta ? beta[c] : 0.0f;
  }
  __syncthreads();
  const int q4 = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c4 = cgi * 32 + q4 * 4;
  if (c4 >= C) return;
  float mu4[4], sc4[4], bt4[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    mu4[e] = s_mu[q4 * 4 + e];
    sc4[e] = s_sc[q4 * 4 + e];
    bt4[e] = s_bt[q4 * 4 + e];
  }
  const int64_t r0 = (int64_t)blockIdx.x * BN_SF_ROWS;
#pragma unroll 4
  for (int it = 0; it < BN_SF_ROWS / 32; ++it) {
    const int64_t r = r0 + it * 32 + rl;
    if (r < M) {
      const float4 vx = *reinterpret_cast<const float4*>(x + r * C + c4);
      float o[4] = {vx.x, vx.y, vx.z, vx.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = bn_fwd_elem(o[e], mu4[e], sc4[e], bt4[e], relu);
      *reinterpret_cast<float4*>(y + r * C + c4) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

__global__ __launch_bounds__(256) void bn_small_bwd_finish_apply_kernel(
    const float* __restrict__ partial, int nblk, int C, int64_t M, const float* __restrict__ x,
    const float* __restrict__ dy, const float* __restrict__ mean, const float* __restrict__ var,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ addend, float eps, int relu,
    float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta, int G) {
  __shared__ double red[2][8][33];
  __shared__ float s_k1[32], s_k2[32];
  const int cgi = blockIdx.y;
  const int cl = threadIdx.x & 31;
  const int c = cgi * 32 + cl;
  const bool own = (threadIdx.x >> 5) == 0 && c < C;
  double T[2];
  bn_small_totals<2>(partial, nblk, C, M, G, c, own, red, T);
  if (own) {
    const float db = (float)T[0], dg = (float)T[1];
    if (blockIdx.x == 0) {
      dbeta[c] = db;
      dgamma[c] = dg;
    }
    const float inv_m = 1.0f / (float)M;      // k1, k2 of bn_bwd_apply_body
    s_k1[cl] = db * inv_m;
    s_k2[cl] = dg * inv_m;
  }
  __syncthreads();
  const int q4 = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c4 = cgi * 32 + q4 * 4;
  if (c4 >= C) return;
  BnBwdCoef k;
  float k1[4], k2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    k.load(e, c4 + e, mean, var, gamma, beta, eps);
    k1[e] = s_k1[q4 * 4 + e];
    k2[e] = s_k2[q4 * 4 + e];
  }
  const int64_t r0 = (int64_t)blockIdx.x * BN_SF_ROWS;
#pragma unroll 2
  for (int it = 0; it < BN_SF_ROWS / 32; ++it) {
    const int64_t r = r0 + it * 32 + rl;
    if (r < M) {
      const float4 vx = *reinterpret_cast<const float4*>(x + r * C + c4);
      const float4 vd = *reinterpret_cast<const float4*>(dy + r * C + c4);
      float4 va = make_float4(0.f, 0.f, 0.f, 0.f);
      if (addend) va = *reinterpret_cast<const float4*>(addend + r * C + c4);
      const float xv[4] = {vx.x, vx.y, vx.z, vx.w}, dv[4] = {vd.x, vd.y, vd.z, vd.w}, av[4] = {va.x, va.y, va.z, va.w};
      float ov[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        ov[e] = bn_bwd_dx(bn_bwd_elem(xv[e], dv[e], k, e, relu), k, e, k1[e], k2[e], 1, addend != nullptr, av[e]);
      *reinterpret_cast<float4*>(dx + r * C + c4) = make_float4(ov[0], ov[1], ov[2], ov[3]);
    }
  }
}

// chunks up to which a level takes finish + apply as ONE launch in which every workgroup redoes the (chunked) finish of its
// channel group: up to WSIS_BN_SMALL_G chunks (default 4: rows < ~10,240 -- level 2 of a scene, level 3 of four; 1: rows
// < 4,096) -- a workgroup re-reads <= 320 partial rows of 32 channels (80 KB from L2) instead of the step paying a launch
// + a kernel boundary per layer and direction.  Same bits as the two launches (the chunk order of the ticketed second
// level).  Read per call.
static int bn_small_gmax() {
  const char* e = getenv("WSIS_BN_SMALL_G");
  const int g = e ? atoi(e) : 4;
  return g < 1 ? 1 : g > 8 ? 8 : g;
}
static bool bn_small_fused_on() {      // WSIS_BN_SMALL_FUSED=0 (read per call): the two launches
  const char* e = getenv("WSIS_BN_SMALL_FUSED");
  return !e || atoi(e) != 0;
}

int bn_nblk(int64_t M, int Cp) { return (int)ceil_div(M > 0 ? M : 1, (int64_t)bn_rows_per_wg(Cp)); }

#if WSIS_EXPERIMENTAL
// ---- the polled producer / consumer form (WSIS_BN_FUSED_APPLY; EXPERIMENTAL build only): statistics finish + apply, and
// backward reduction finish + apply, in ONE launch.  The first G * ceil(C/32) workgroups run the chunk stage (tickets
// included); the workgroup that completes the last channel group publishes the launch's epoch in `flag`; every workgroup
// waits for it and then applies.  The grid is at most 512 workgroups of 256 threads (two per CU): all of them are
// resident, the waiting ones cannot keep the working ones off the machine.  Same arithmetic as the two launches
// (bn_chunk_stage, bn_apply_body / bn_bwd_apply_body): identical results.
constexpr int BN_POLL_SLEEP = 12;      // x 64 cycles
constexpr unsigned long long BN_SPIN_LIMIT = 200000000ull;      // s_memrealtime ticks (100 MHz): 2 s

// every workgroup of a producer / consumer launch: wait until the producers have published (flag != 0), bounded -- a
// launch whose producers never become resident sets `err` and goes on instead of hanging the device --, then the
// workgroup that leaves the wait last puts flag and counter back to zero for the next launch on this slot
__device__ __forceinline__ void bn_wait_published(SyncSlot* s) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(&s->flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
      __builtin_amdgcn_s_sleep(BN_POLL_SLEEP);
      if (__builtin_amdgcn_s_memrealtime() - t0 > BN_SPIN_LIMIT) {
        __hip_atomic_store(&s->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
    const unsigned l = atomicAdd(&s->left, 1u);
    if (l == gridDim.x - 1) {
      __hip_atomic_store(&s->left, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&s->flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
}
// a workgroup that wrote the result of one channel group (`fin`); the last such group publishes
__device__ __forceinline__ void bn_publish(bool fin, SyncSlot* s, int CG) {
  if (!fin) return;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned d = atomicAdd(&s->done, 1u);
    if (d == (unsigned)CG - 1) {
      __hip_atomic_store(&s->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence();
      __hip_atomic_store(&s->flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ __launch_bounds__(256) void bn_finalize_apply_kernel(
    const float* __restrict__ partial, int nblk, int C, int64_t M, double* __restrict__ chunk, int G,
    float* mean, float* var, float* __restrict__ running_mean,
    float* __restrict__ running_var, float momentum, SyncSlot* __restrict__ sync, const float* __restrict__ x,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu, float* __restrict__ y) {
  __shared__ double red[3][8][33];
  __shared__ int s_last;
  const int CG = (C + 31) / 32;
  if ((int)blockIdx.x < G * CG)
    bn_publish(bn_chunk_centred_stage(partial, nblk, C, M, chunk, mean, var, running_mean, running_var, momentum,
                                      sync->ticket, (int)blockIdx.x % G, G, (int)blockIdx.x / G, red, s_last),
               sync, CG);
  bn_wait_published(sync);    // relaxed polls a few hundred ns apart (hundreds of pollers on one word)
  bn_apply_body<true>(x, mean, var, gamma, beta, eps, relu, y, M, C);
}

__global__ __launch_bounds__(256) void bn_bwd_finish_apply_kernel(
    const float* __restrict__ partial, int nblk, int C, double* __restrict__ chunk, int G, float* dbeta, float* dgamma,
    SyncSlot* __restrict__ sync, const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ addend, float eps, int relu, float* __restrict__ dx, int64_t M) {
  __shared__ double red[2][8][33];
  __shared__ int s_last;
  const int CG = (C + 31) / 32;
  if ((int)blockIdx.x < G * CG)
    bn_publish(bn_sum_chunk_stage(partial, nblk, C, chunk, dbeta, dgamma, sync->ticket, (int)blockIdx.x % G, G,
                                  (int)blockIdx.x / G, red, s_last),
               sync, CG);
  bn_wait_published(sync);
  bn_bwd_apply_body<true>(x, dy, mean, var, gamma, beta, dgamma, dbeta, addend, eps, relu, 1, dx, M, C);
}

// grid of a producer-consumer launch over M x C elements: every workgroup resident (<= 2 per CU of this device),
// a multiple of the channel groups; 0 when the one-launch form does not apply
static int bn_fused_grid(int64_t M, int C, int need_chunk_wgs, int which = 0) {
  // read per call (a test switches the form on): WSIS_BN_FUSED_APPLY for both directions, WSIS_BN_FUSED_FWD / _BWD per
  // direction.  Default OFF since round 3: with the flag / ticket words in caller slots (one more arrival counter per
  // workgroup) and the convolutions on one-launch plans the two-launch form measures faster -- 10.37 / 10.38 ms per C2
  // step against 10.59 / 10.63 with both directions fused, 10.48 / 10.46 and 10.50 / 10.53 with one of them
  // (alternating runs on one box) -- and no workgroup of the default path ever waits for another one inside a launch
  const char* e = getenv("WSIS_BN_FUSED_APPLY");
  const int on = e ? atoi(e) : 0;
  const char* ed = getenv(which ? "WSIS_BN_FUSED_BWD" : "WSIS_BN_FUSED_FWD");
  const int on_dir = ed ? atoi(ed) : on;
  const char* g = tune_env("WSIS_BN_FUSED_GRID");
  int gmax = g ? atoi(g) : 256;
  if (gmax < 64 || gmax > 512) gmax = 256;
  int n_cu = 0;
  {   // per call: the CU count of the CURRENT device (cheap attribute query, no cache shared between devices)
    int dev = 0, v = 0;
    n_cu = (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) ? v : 0;
  }
  if (!on_dir || (C & 3) != 0) return 0;
  const int cw = C >> 2;
  const int64_t work = (M * C) >> 2;
  int gcap = (work > 600000 && gmax == 256) ? 512 : gmax;     // level 0: two workgroups per CU for the apply pass
  if (gcap > 2 * n_cu) gcap = 2 * n_cu;
  if (gcap < 1) return 0;
  int grid = gcap - (gcap % cw);
  const int need = grid_for(work, 256);
  if (need < grid) {
    grid = need;
    if (grid > cw) grid -= grid % cw;
  }
  return (grid >= need_chunk_wgs && grid >= 1) ? grid : 0;
}
#endif  // WSIS_EXPERIMENTAL

// ---- launch plans

// grid of an apply pass over M x C elements, as vector items (quads where C is a multiple of 4) in channel groups: eight
// items per thread (four trips of two) where that still leaves 512 workgroups, else one workgroup per 256 items up to
// 512 -- rounded down to a multiple of the channel groups (a thread then keeps its channel group for its whole walk).
// The round-4 grid (one item per thread up to 2,048 workgroups) left a level-0 thread 2.3 items -- a third trip that a
// third of the threads take -- and a level-1 thread ONE: nothing in flight behind it.  tools/bn_bench.py, apply /
// backward apply in us: 153,685 x 32: 9.0 / 14.7 -> 7.4 / 12.0; 26,819 x 64: 9.5 / 16.4 -> 4.7 / 9.1; 26,819 x 128:
// 11.3 / 18.4 -> 6.5 / 10.2; small levels unchanged.
static int bn_apply_grid(int64_t M, int C) {
  const bool vec = (C & 3) == 0;
  const int64_t work = vec ? (M * C) >> 2 : M * C;
  const int cw = vec ? C >> 2 : C;
  int64_t g = ceil_div(work, (int64_t)256 * 8);
  if (g < 512) {
    g = ceil_div(work, 256);
    if (g > 512) g = 512;
  }
  if (g > 16384) g = 16384;
  if (g < 1) g = 1;
  if (g > cw) g -= g % cw;
  return (int)g;
}

template <typename T, typename TO>
static int launch_bn_bwd_apply(const T* d_x, const T* d_dy, const float* d_mean, const float* d_var,
                               const float* d_gamma, const float* d_beta, const float* d_dgamma, const float* d_dbeta,
                               const T* d_addend, float eps, int relu, int training, TO* d_dx, int64_t M, int C,
                               hipStream_t st) {
  hipLaunchKernelGGL((bn_bwd_apply_kernel<T, TO>), dim3(bn_apply_grid(M, C)), dim3(256), 0, st, d_x, d_dy, d_mean, d_var,
                     d_gamma, d_beta, d_dgamma, d_dbeta, d_addend, eps, relu, training, d_dx, M, C);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

// The launch plan of the stand-alone statistics (wsis_bn_stats, wsis_bn_stats_lp) and of the stand-alone backward
// reduction (wsis_bn_bwd, wsis_bn_bwd_lp): one launch up to bn_small_rows() rows, partial + final above.  The element
// type changes the loads only: grids, trees and the branch by M are the same for fp32 and 16-bit tensors.
template <typename T>
static int bn_stats_run(const T* d_x, int64_t M, int C, float* d_mean, float* d_var, float* d_running_mean,
                        float* d_running_var, float momentum, void* d_ws, hipStream_t st) {
  const int Cp = (C + 3) / 4 * 4;
  const int nblk = bn_nblk(M, Cp);
  float* partial = static_cast<float*>(d_ws);
  WSIS_REQUIRE(Cp / 4 <= BN_THREADS, "C > 1024 is not supported");
  if (M <= bn_small_rows()) {
    hipLaunchKernelGGL(bn_stats_small_kernel<T>, dim3(Cp / 4), dim3(BN_SMALL_THREADS), 0, st, d_x, M, C, d_mean, d_var,
                       d_running_mean, d_running_var, momentum);
    WSIS_LAUNCH_CHECK();
    return WSIS_OK;
  }
  hipLaunchKernelGGL(bn_stats_partial_kernel<T>, dim3(nblk), dim3(BN_THREADS), 0, st, d_x, M, C, Cp, partial);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_stats_final_kernel<T>, dim3(C), dim3(64), 0, st, partial, nblk, C, Cp, M, d_x, d_mean, d_var,
                     d_running_mean, d_running_var, momentum);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}
template <typename T>
static int bn_bwd_reduce_run(const T* d_x, const T* d_dy, const float* d_mean, const float* d_var, const float* d_gamma,
                             const float* d_beta, float eps, int relu, float* d_dgamma, float* d_dbeta, int64_t M, int C,
                             void* d_ws, hipStream_t st) {
  const int Cp = (C + 3) / 4 * 4;
  const int nblk = bn_nblk(M, Cp);
  float* partial = static_cast<float*>(d_ws);
  WSIS_REQUIRE(Cp / 4 <= BN_THREADS, "C > 1024 is not supported");
  if (M <= bn_small_rows()) {
    hipLaunchKernelGGL(bn_bwd_small_kernel<T>, dim3(Cp / 4), dim3(BN_SMALL_THREADS), 0, st, d_x, d_dy, d_mean, d_var,
                       d_gamma, d_beta, eps, relu, M, C, d_dgamma, d_dbeta);
    WSIS_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(bn_bwd_partial_kernel<T>, dim3(nblk), dim3(BN_THREADS), 0, st, d_x, d_dy, d_mean, d_var, d_gamma,
                       d_beta, eps, relu, M, C, Cp, partial);
    WSIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(C), dim3(64), 0, st, partial, nblk, C, Cp, d_dgamma, d_dbeta);
    WSIS_LAUNCH_CHECK();
  }
  return WSIS_OK;
}
// the apply pass of a 16-bit backward (wsis_bn_bwd_lp, wsis_bn_bwd_apply_lp): dx as TO = T, or as float when out_fp32
template <typename T>
static int bn_bwd_apply_lp_run(const void* d_x, const void* d_dy, const float* d_mean, const float* d_var,
                               const float* d_gamma, const float* d_beta, const float* d_dgamma, const float* d_dbeta,
                               const void* d_addend, float eps, int relu, int training, void* d_dx, int out_fp32, int64_t M,
                               int C, hipStream_t st) {
  const T *x = static_cast<const T*>(d_x), *dy = static_cast<const T*>(d_dy), *ad = static_cast<const T*>(d_addend);
  if (out_fp32)
    return launch_bn_bwd_apply(x, dy, d_mean, d_var, d_gamma, d_beta, d_dgamma, d_dbeta, ad, eps, relu, training,
                               static_cast<float*>(d_dx), M, C, st);
  return launch_bn_bwd_apply(x, dy, d_mean, d_var, d_gamma, d_beta, d_dgamma, d_dbeta, ad, eps, relu, training,
                             static_cast<T*>(d_dx), M, C, st);
}
// reduction, then dx (d_dx == nullptr: none)
template <typename T>
static int bn_bwd_lp_run(const void* d_x, const void* d_dy, const float* d_mean, const float* d_var, const float* d_gamma,
                         const float* d_beta, float eps, int relu, int training, void* d_dx, int out_fp32,
                         float* d_dgamma, float* d_dbeta, const void* d_addend, int64_t M, int C, void* d_ws,
                         hipStream_t st) {
  const int rc = bn_bwd_reduce_run(static_cast<const T*>(d_x), static_cast<const T*>(d_dy), d_mean, d_var, d_gamma, d_beta,
                                   eps, relu, d_dgamma, d_dbeta, M, C, d_ws, st);
  if (rc != WSIS_OK || !d_dx) return rc;
  return bn_bwd_apply_lp_run<T>(d_x, d_dy, d_mean, d_var, d_gamma, d_beta, d_dgamma, d_dbeta, d_addend, eps, relu, training,
                                d_dx, out_fp32, M, C, st);
}

// ticket row of a two-level reduction: the caller's sync slot (nullptr without one, or with WSIS_BN_TICKET=0: the finish
// runs as a second launch)
static unsigned* bn_tickets(void* d_sync) {
  static const int on = [] {
    const char* e = tune_env("WSIS_BN_TICKET");
    return e ? atoi(e) : 1;
  }();
  if (!on || !d_sync) return nullptr;
  return static_cast<SyncSlot*>(d_sync)->ticket;
}

static bool bn_aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}
static void* bn_align256(void* p) {
  return reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255);
}

// the two-level reductions of per-slice partials (wsis_bn_stats_finalize, _finalize_apply, wsis_bn_bwd_from_partials): G
// chunks x CG channel groups, chunk rows in the caller's workspace (needed from two chunks on), tickets in its sync slot
struct BnCentredPlan {
  int G, CG;
  bool ws_ok;
  double* chunk;
  unsigned* tickets;
};
static BnCentredPlan bn_centred_plan(int64_t n_part, int C, void* d_ws, int64_t ws_bytes, void* d_sync) {
  BnCentredPlan p;
  p.G = bn_fin_chunks(n_part);
  p.CG = (C + 31) / 32;
  p.ws_ok = p.G == 1 || (d_ws && ws_bytes >= wsis_bn_stats_finalize_workspace_bytes(n_part, C));
  p.chunk = static_cast<double*>(bn_align256(d_ws));
  p.tickets = bn_tickets(d_sync);
  return p;
}
// few chunks: finish + apply in one launch without any hand-off (bn_small_*_finish_apply_kernel: float4 rows)
static bool bn_small_fused_ok(const BnCentredPlan& p, int C, std::initializer_list<const void*> rows) {
  return p.G <= bn_small_gmax() && (p.G == 1 || p.tickets) && (C & 3) == 0 && bn_small_fused_on() && bn_aligned16(rows);
}

// ---- statistics shared across ranks (wsis_bn_sync_*): what a synced layer does on either side of its collective, one
// thread per channel, fp64, the ranks in ascending order -- every operation an IEEE + - * / or a rounding cast
// (-ffp-contract=off), so a host restatement of the same expressions gives the same bits
constexpr int BN_SYNC_THREADS = 64;

__global__ __launch_bounds__(BN_SYNC_THREADS) void bn_sync_pack_kernel(const float* __restrict__ mean,
                                                                       const float* __restrict__ var, int64_t M, int C,
                                                                       double* __restrict__ out) {
  const int c = blockIdx.x * BN_SYNC_THREADS + threadIdx.x;
  if (c >= C) return;
  out[c] = M > 0 ? (double)mean[c] : 0.0;
  out[C + c] = M > 0 ? (double)var[c] : 0.0;
  if (c == 0) out[2 * C] = (double)M;
}

__global__ __launch_bounds__(BN_SYNC_THREADS) void bn_sync_combine_kernel(const double* __restrict__ g, int R, int C,
                                                                          float* __restrict__ mean, float* __restrict__ var,
                                                                          float* __restrict__ running_mean,
                                                                          float* __restrict__ running_var, float momentum,
                                                                          double* __restrict__ count) {
  const int c = blockIdx.x * BN_SYNC_THREADS + threadIdx.x;
  if (c >= C) return;
  const int64_t P = 2 * (int64_t)C + 1;      // one rank's row: mean[C], var[C], rows
  double N = g[2 * C];
  for (int r = 1; r < R; ++r) N += g[r * P + 2 * C];
  if (c == 0) count[0] = N;
  if (!(N > 0.0)) {      // no rank holds a row: nothing to normalise, the running statistics stay
    mean[c] = 0.0f;
    var[c] = 0.0f;
    return;
  }
  double s = g[c] * g[2 * C];
  for (int r = 1; r < R; ++r) s += g[r * P + c] * g[r * P + 2 * C];
  const double mean64 = s / N;
  double q = 0.0;
  for (int r = 0; r < R; ++r) {
    const double dm = g[r * P + c] - mean64;
    const double t = (g[r * P + C + c] + dm * dm) * g[r * P + 2 * C];
    q = r == 0 ? t : q + t;
  }
  const double var64 = q / N;
  const float m32 = (float)mean64;
  mean[c] = m32;
  var[c] = (float)var64;
  if (running_mean) {
    const double n1 = N - 1.0 > 1.0 ? N - 1.0 : 1.0;
    running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * m32;
    running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)(var64 * N / n1);
  }
}

__global__ __launch_bounds__(BN_SYNC_THREADS) void bn_sync_sums_pack_kernel(const float* __restrict__ dgamma,
                                                                            const float* __restrict__ dbeta, int C,
                                                                            double* __restrict__ out) {
  const int c = blockIdx.x * BN_SYNC_THREADS + threadIdx.x;
  if (c >= C) return;
  out[c] = dgamma ? (double)dgamma[c] : 0.0;
  out[C + c] = dbeta ? (double)dbeta[c] : 0.0;
}

__global__ __launch_bounds__(BN_SYNC_THREADS) void bn_sync_sums_scale_kernel(const double* __restrict__ sums, int64_t M,
                                                                             const double* __restrict__ count, int C,
                                                                             float* __restrict__ sum_dz_xhat,
                                                                             float* __restrict__ sum_dz) {
  const int c = blockIdx.x * BN_SYNC_THREADS + threadIdx.x;
  if (c >= C) return;
  const double k = (double)M / count[0];      // the apply pass divides by the local row count
  sum_dz_xhat[c] = (float)(sums[c] * k);
  sum_dz[c] = (float)(sums[C + c] * k);
}

inline unsigned bn_sync_grid(int C) { return (unsigned)((C + BN_SYNC_THREADS - 1) / BN_SYNC_THREADS); }

}  // namespace

extern "C" {

int64_t wsis_bn_workspace_bytes(int64_t M, int32_t C) {
  if (M < 0 || C < 1) return -1;
  const int64_t Cp = (C + 3) / 4 * 4;
  return (int64_t)bn_nblk(M, (int)Cp) * 2 * Cp * (int64_t)sizeof(float) + 256;
}

int wsis_bn_stats(const float* d_x, int64_t M, int32_t C, float* d_mean, float* d_var, float* d_running_mean,
                  float* d_running_var, float momentum, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(M >= 1 && C >= 1 && d_x && d_mean && d_var && d_ws, "bad args");
  WSIS_REQUIRE(ws_bytes >= wsis_bn_workspace_bytes(M, C), "workspace too small");
  WSIS_REQUIRE((d_running_mean == nullptr) == (d_running_var == nullptr), "running stats come in pairs");
  return bn_stats_run(d_x, M, C, d_mean, d_var, d_running_mean, d_running_var, momentum, d_ws, as_stream(stream));
}

// the 16-bit tensors of a pass: rows of C % 8 == 0 elements (16 bytes and multiples), 16-byte aligned bases
static bool bn_lp_domain(int C, int dtype, std::initializer_list<const void*> ps) {
  return (dtype == 0 || dtype == 1) && C % 8 == 0 && C <= 1024 && bn_aligned16(ps);
}

int wsis_bn_stats_lp(const void* d_x, int64_t M, int32_t C, float* d_mean, float* d_var, float* d_running_mean,
                     float* d_running_var, float momentum, void* d_ws, int64_t ws_bytes, int32_t dtype, void* stream) {
  WSIS_REQUIRE(M >= 1 && C >= 1 && d_x && d_mean && d_var && d_ws, "bad args");
  WSIS_REQUIRE(bn_lp_domain(C, dtype, {d_x}), "16-bit BatchNorm: dtype 0 / 1, C % 8 == 0, C <= 1024, 16-byte aligned x");
  WSIS_REQUIRE(ws_bytes >= wsis_bn_workspace_bytes(M, C), "workspace too small");
  WSIS_REQUIRE((d_running_mean == nullptr) == (d_running_var == nullptr), "running stats come in pairs");
  hipStream_t st = as_stream(stream);
  if (dtype == 0)
    return bn_stats_run(static_cast<const __bf16*>(d_x), M, C, d_mean, d_var, d_running_mean, d_running_var, momentum,
                        d_ws, st);
  return bn_stats_run(static_cast<const _Float16*>(d_x), M, C, d_mean, d_var, d_running_mean, d_running_var, momentum,
                      d_ws, st);
}

// ---- column sums of x [M, C] (bias gradient of a Linear layer over M rows): two levels in ONE launch, fixed order.
// 256 threads = (C/4 float4 column lanes) x (row lanes); every workgroup sums a block of rows, the one that arrives
// last adds the block results in block order.

// IN / OUT: the rows read (IN) or the row written (OUT) are handed between workgroups of this launch -> sc1 accesses
__device__ __forceinline__ void colsum_block(const bool IN, const bool OUT, const float* __restrict__ x, int64_t lo,
                                             int64_t hi, int C4, float4* red, float* __restrict__ out) {
  const int RL = 256 / C4;
  const int cl = threadIdx.x % C4, rl = threadIdx.x / C4;
  float4 a = {0.f, 0.f, 0.f, 0.f};
  if (rl < RL) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
#pragma unroll 8
    for (int64_t r = lo + rl; r < hi; r += RL) {
      float4 v;
      if (IN) {
        const float* p = x + (r * C4 + cl) * 4;
        v = make_float4(ld_sc1(p), ld_sc1(p + 1), ld_sc1(p + 2), ld_sc1(p + 3));
      } else {
        v = x4[r * C4 + cl];
      }
      a.x += v.x;
      a.y += v.y;
      a.z += v.z;
      a.w += v.w;
    }
    red[rl * C4 + cl] = a;
  }
  __syncthreads();
  if (threadIdx.x < C4) {
    float4 s = red[threadIdx.x];
    for (int j = 1; j < RL; ++j) {      // fixed order
      const float4 v = red[j * C4 + threadIdx.x];
      s.x += v.x;
      s.y += v.y;
      s.z += v.z;
      s.w += v.w;
    }
    if (OUT) {
      float* p = out + threadIdx.x * 4;
      st_sc1(p, s.x);
      st_sc1(p + 1, s.y);
      st_sc1(p + 2, s.z);
      st_sc1(p + 3, s.w);
    } else {
      reinterpret_cast<float4*>(out)[threadIdx.x] = s;
    }
  }
}

__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, int64_t M, int C, int64_t per,
                                                     float* __restrict__ chunk, float* __restrict__ out,
                                                     unsigned* __restrict__ ticket) {
  __shared__ float4 red[256];
  __shared__ int s_last;
  const int C4 = C >> 2;
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < M ? lo + per : M;
  if (gridDim.x == 1) {
    colsum_block(false, false, x, lo, hi, C4, red, out);
    return;
  }
  colsum_block(false, true, x, lo, hi, C4, red, chunk + (int64_t)blockIdx.x * C);
  wait_stores_left();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = atomicAdd(ticket, 1u);
    s_last = t == gridDim.x - 1;
    if (s_last) *ticket = 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __syncthreads();            // `red` of the first pass has been read by everyone
  colsum_block(true, false, chunk, 0, gridDim.x, C4, red, out);
}

// G chunks of `per` rows.  <= 128 chunks: every chunk ends in an agent-scope ticket add on ONE word (~50 ns each,
// serialised across the XCDs) and the last workgroup walks the chunk rows -- 781 chunks of 256 rows made the
// [199790, 20] bias gradient 58 us
static void colsum_plan(int64_t M, int64_t* per, int64_t* G) {
  *per = (M + 127) / 128;
  if (*per < 256) *per = 256;
  *G = (M + *per - 1) / *per;
}

int64_t wsis_bn_stats_finalize_workspace_bytes(int64_t n_part, int32_t C) {
  return (int64_t)bn_fin_chunks(n_part) * 3 * C * (int64_t)sizeof(double) + 256;
}

int wsis_bn_stats_finalize(const float* d_partials, int64_t n_part, int64_t M, int32_t C, float* d_mean, float* d_var,
                           float* d_running_mean, float* d_running_var, float momentum, void* d_ws, int64_t ws_bytes,
                           void* d_sync, void* stream) {
  WSIS_REQUIRE(n_part >= 1 && M >= 1 && C >= 1 && d_partials && d_mean && d_var, "bad args");
  WSIS_REQUIRE(n_part < ((int64_t)1 << 31), "too many partials");
  WSIS_REQUIRE((d_running_mean == nullptr) == (d_running_var == nullptr), "running stats come in pairs");
  WSIS_REQUIRE(n_part == (M + 31) / 32, "one partial per 32-row slice");
  const BnCentredPlan p = bn_centred_plan(n_part, C, d_ws, ws_bytes, d_sync);
  WSIS_REQUIRE(p.ws_ok, "workspace too small");
  WSIS_REQUIRE(C <= 512, "more than 512 channels");
  hipLaunchKernelGGL(bn_stats_chunk_centred_kernel, dim3(p.G, p.CG), dim3(256), 0, as_stream(stream), d_partials,
                     (int)n_part, C, M, p.chunk, d_mean, d_var, d_running_mean, d_running_var, momentum, p.tickets);
  WSIS_LAUNCH_CHECK();
  if (p.G > 1 && !p.tickets) {
    hipLaunchKernelGGL(bn_stats_final_centred_kernel, dim3((C + 3) / 4), dim3(256), 0, as_stream(stream), p.chunk, p.G, C,
                       M, d_mean, d_var, d_running_mean, d_running_var, momentum);
    WSIS_LAUNCH_CHECK();
  }
  return WSIS_OK;
}

int wsis_bn_stats_finalize_apply(const float* d_partials, int64_t n_part, int64_t M, int32_t C, float* d_mean,
                                 float* d_var, float* d_running_mean, float* d_running_var, float momentum,
                                 const float* d_x, const float* d_gamma, const float* d_beta, float eps, int32_t relu,
                                 float* d_y, void* d_ws, int64_t ws_bytes, void* d_sync, void* stream) {
  WSIS_REQUIRE(n_part >= 1 && M >= 1 && C >= 1 && d_partials && d_mean && d_var && d_x && d_y, "bad args");
  WSIS_REQUIRE(n_part == (M + 31) / 32 && n_part < ((int64_t)1 << 31), "one partial per 32-row slice");
  WSIS_REQUIRE(C <= 512, "more than 512 channels");
  hipStream_t st = as_stream(stream);
  const BnCentredPlan p = bn_centred_plan(n_part, C, d_ws, ws_bytes, d_sync);
  WSIS_REQUIRE(p.ws_ok, "workspace too small");
  if (bn_small_fused_ok(p, C, {d_x, d_y})) {
    hipLaunchKernelGGL(bn_small_finish_apply_kernel, dim3((unsigned)ceil_div(M, BN_SF_ROWS), (unsigned)p.CG), dim3(256), 0,
                       st, d_partials, (int)n_part, (int)C, M, d_mean, d_var, d_running_mean, d_running_var, momentum, d_x,
                       d_gamma, d_beta, eps, (int)relu, d_y, p.G);
    WSIS_LAUNCH_CHECK();
    return WSIS_OK;
  }
#if WSIS_EXPERIMENTAL
  // the polled one-launch form needs: a sync slot (tickets + flag), every workgroup resident, vector rows
  if (const int grid = p.tickets ? bn_fused_grid(M, C, p.G * p.CG) : 0) {
    hipLaunchKernelGGL(bn_finalize_apply_kernel, dim3(grid), dim3(256), 0, st, d_partials, (int)n_part, (int)C, M, p.chunk,
                       p.G, d_mean, d_var, d_running_mean, d_running_var, momentum, static_cast<SyncSlot*>(d_sync), d_x,
                       d_gamma, d_beta, eps, (int)relu, d_y);
    WSIS_LAUNCH_CHECK();
    return WSIS_OK;
  }
#endif
  const int rc = wsis_bn_stats_finalize(d_partials, n_part, M, C, d_mean, d_var, d_running_mean, d_running_var, momentum,
                                        d_ws, ws_bytes, d_sync, stream);
  if (rc != WSIS_OK) return rc;
  return wsis_bn_apply(d_x, d_mean, d_var, d_gamma, d_beta, eps, relu, d_y, M, C, stream);
}

int wsis_bn_apply(const float* d_x, const float* d_mean, const float* d_var, const float* d_gamma,
                  const float* d_beta, float eps, int32_t relu, float* d_y, int64_t M, int32_t C, void* stream) {
  WSIS_REQUIRE(M >= 0 && C >= 1, "bad sizes");
  if (M == 0) return WSIS_OK;
  WSIS_REQUIRE(d_x && d_mean && d_var && d_y, "null pointer");
  hipLaunchKernelGGL(bn_apply_kernel, dim3(bn_apply_grid(M, C)), dim3(256), 0, as_stream(stream), d_x, d_mean, d_var,
                     d_gamma, d_beta, eps, relu, d_y, M, C);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_bn_apply_lp(const void* d_x, const float* d_mean, const float* d_var, const float* d_gamma,
                     const float* d_beta, float eps, int32_t relu, void* d_y, int32_t out_fp32, int64_t M, int32_t C,
                     int32_t dtype, void* stream) {
  WSIS_REQUIRE(M >= 0 && C >= 1, "bad sizes");
  WSIS_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (bf16) or 1 (fp16)");
  if (M == 0) return WSIS_OK;
  WSIS_REQUIRE(d_x && d_mean && d_var && d_y, "null pointer");
  const int grid = bn_apply_grid(M, C);      // the grid of wsis_bn_apply: the same walk over the same quads
  if ((C & 3) == 0)
    WSIS_REQUIRE((reinterpret_cast<uintptr_t>(d_x) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(d_y) & (out_fp32 ? 15 : 7)) == 0,
                 "x and y must be aligned to a quad of elements");
  hipStream_t st = as_stream(stream);
  if (dtype == 0)
    launch_bn_apply_lp<__bf16>(d_x, d_mean, d_var, d_gamma, d_beta, eps, relu, d_y, out_fp32, M, C, grid, st);
  else
    launch_bn_apply_lp<_Float16>(d_x, d_mean, d_var, d_gamma, d_beta, eps, relu, d_y, out_fp32, M, C, grid, st);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_bn_bwd_from_partials(const float* d_partials, int64_t n_part, const float* d_x, const float* d_dy,
                              const float* d_mean, const float* d_var, const float* d_gamma, const float* d_beta,
                              float eps, int32_t relu, float* d_dx, float* d_dgamma, float* d_dbeta,
                              const float* d_addend, int64_t M, int32_t C, void* d_ws, int64_t ws_bytes, void* d_sync,
                              void* stream) {
  WSIS_REQUIRE(M >= 1 && C >= 1 && d_partials && d_x && d_dy && d_mean && d_var && d_dgamma && d_dbeta, "bad args");
  WSIS_REQUIRE(n_part == (M + 31) / 32 && n_part < ((int64_t)1 << 31), "one partial per 32-row slice");
  const BnCentredPlan p = bn_centred_plan(n_part, C, d_ws, ws_bytes, d_sync);
  WSIS_REQUIRE(p.ws_ok, "workspace too small");
  hipStream_t st = as_stream(stream);
  WSIS_REQUIRE(C <= 512, "more than 512 channels");
  if (d_dx && bn_small_fused_ok(p, C, {d_x, d_dy, d_dx, d_addend})) {
    hipLaunchKernelGGL(bn_small_bwd_finish_apply_kernel, dim3((unsigned)ceil_div(M, BN_SF_ROWS), (unsigned)p.CG), dim3(256),
                       0, st, d_partials, (int)n_part, (int)C, M, d_x, d_dy, d_mean, d_var, d_gamma, d_beta, d_addend, eps,
                       (int)relu, d_dx, d_dgamma, d_dbeta, p.G);
    WSIS_LAUNCH_CHECK();
    return WSIS_OK;
  }
#if WSIS_EXPERIMENTAL
  // reduction finish + apply in one polled launch (the form of wsis_bn_stats_finalize_apply)
  if (const int grid = d_dx && p.tickets ? bn_fused_grid(M, C, p.G * p.CG, 1) : 0) {
    hipLaunchKernelGGL(bn_bwd_finish_apply_kernel, dim3(grid), dim3(256), 0, st, d_partials, (int)n_part, (int)C, p.chunk,
                       p.G, d_dbeta, d_dgamma, static_cast<SyncSlot*>(d_sync), d_x, d_dy, d_mean, d_var, d_gamma, d_beta,
                       d_addend, eps, (int)relu, d_dx, M);
    WSIS_LAUNCH_CHECK();
    return WSIS_OK;
  }
#endif
  hipLaunchKernelGGL(bn_sum_chunk_kernel, dim3(p.G, p.CG), dim3(256), 0, st, d_partials, (int)n_part, C, p.chunk, d_dbeta,
                     d_dgamma, p.tickets);
  WSIS_LAUNCH_CHECK();
  if (p.G > 1 && !p.tickets) {
    hipLaunchKernelGGL(bn_sum_final_kernel, dim3((C + 3) / 4), dim3(256), 0, st, p.chunk, p.G, C, d_dbeta, d_dgamma);
    WSIS_LAUNCH_CHECK();
  }
  if (!d_dx) return WSIS_OK;
  return launch_bn_bwd_apply(d_x, d_dy, d_mean, d_var, d_gamma, d_beta, d_dgamma, d_dbeta, d_addend, eps, relu, 1, d_dx, M,
                             C, st);
}

int wsis_bn_bwd_apply(const float* d_x, const float* d_dy, const float* d_mean, const float* d_var,
                      const float* d_gamma, const float* d_beta, const float* d_sum_dz_xhat, const float* d_sum_dz,
                      float eps, int32_t relu, float* d_dx, const float* d_addend, int64_t M, int32_t C, void* stream) {
  WSIS_REQUIRE(M >= 1 && C >= 1 && d_x && d_dy && d_mean && d_var && d_sum_dz_xhat && d_sum_dz && d_dx, "bad args");
  return launch_bn_bwd_apply(d_x, d_dy, d_mean, d_var, d_gamma, d_beta, d_sum_dz_xhat, d_sum_dz, d_addend, eps, relu, 1,
                             d_dx, M, C, as_stream(stream));
}

int wsis_bn_bwd(const float* d_x, const float* d_dy, const float* d_mean, const float* d_var,
                const float* d_gamma, const float* d_beta, float eps, int32_t relu, int32_t training,
                float* d_dx, float* d_dgamma, float* d_dbeta, const float* d_addend, int64_t M, int32_t C, void* d_ws,
                int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(M >= 1 && C >= 1 && d_x && d_dy && d_mean && d_var && d_dgamma && d_dbeta && d_ws, "bad args");
  WSIS_REQUIRE(ws_bytes >= wsis_bn_workspace_bytes(M, C), "workspace too small");
  hipStream_t st = as_stream(stream);
  const int rc = bn_bwd_reduce_run(d_x, d_dy, d_mean, d_var, d_gamma, d_beta, eps, relu, d_dgamma, d_dbeta, M, C, d_ws, st);
  if (rc != WSIS_OK || !d_dx) return rc;
  return launch_bn_bwd_apply(d_x, d_dy, d_mean, d_var, d_gamma, d_beta, d_dgamma, d_dbeta, d_addend, eps, relu, training,
                             d_dx, M, C, st);
}

int wsis_bn_bwd_lp(const void* d_x, const void* d_dy, const float* d_mean, const float* d_var, const float* d_gamma,
                   const float* d_beta, float eps, int32_t relu, int32_t training, void* d_dx, int32_t out_fp32,
                   float* d_dgamma, float* d_dbeta, const void* d_addend, int64_t M, int32_t C, int32_t dtype, void* d_ws,
                   int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(M >= 1 && C >= 1 && d_x && d_dy && d_mean && d_var && d_dgamma && d_dbeta && d_ws, "bad args");
  WSIS_REQUIRE(bn_lp_domain(C, dtype, {d_x, d_dy, d_dx, d_addend}),
               "16-bit BatchNorm: dtype 0 / 1, C % 8 == 0, C <= 1024, 16-byte aligned tensors");
  WSIS_REQUIRE(ws_bytes >= wsis_bn_workspace_bytes(M, C), "workspace too small");
  hipStream_t st = as_stream(stream);
  if (dtype == 0)
    return bn_bwd_lp_run<__bf16>(d_x, d_dy, d_mean, d_var, d_gamma, d_beta, eps, relu, training, d_dx, out_fp32, d_dgamma,
                                 d_dbeta, d_addend, M, C, d_ws, st);
  return bn_bwd_lp_run<_Float16>(d_x, d_dy, d_mean, d_var, d_gamma, d_beta, eps, relu, training, d_dx, out_fp32, d_dgamma,
                                 d_dbeta, d_addend, M, C, d_ws, st);
}

int wsis_bn_bwd_apply_lp(const void* d_x, const void* d_dy, const float* d_mean, const float* d_var, const float* d_gamma,
                         const float* d_beta, const float* d_sum_dz_xhat, const float* d_sum_dz, float eps, int32_t relu,
                         void* d_dx, int32_t out_fp32, const void* d_addend, int64_t M, int32_t C, int32_t dtype,
                         void* stream) {
  WSIS_REQUIRE(M >= 1 && C >= 1 && d_x && d_dy && d_mean && d_var && d_sum_dz_xhat && d_sum_dz && d_dx, "bad args");
  WSIS_REQUIRE(bn_lp_domain(C, dtype, {d_x, d_dy, d_dx, d_addend}),
               "16-bit BatchNorm: dtype 0 / 1, C % 8 == 0, C <= 1024, 16-byte aligned tensors");
  hipStream_t st = as_stream(stream);
  if (dtype == 0)
    return bn_bwd_apply_lp_run<__bf16>(d_x, d_dy, d_mean, d_var, d_gamma, d_beta, d_sum_dz_xhat, d_sum_dz, d_addend, eps,
                                       relu, 1, d_dx, out_fp32, M, C, st);
  return bn_bwd_apply_lp_run<_Float16>(d_x, d_dy, d_mean, d_var, d_gamma, d_beta, d_sum_dz_xhat, d_sum_dz, d_addend, eps,
                                       relu, 1, d_dx, out_fp32, M, C, st);
}

int wsis_bn_sync_pack(const float* d_mean, const float* d_var, int64_t M, int32_t C, double* d_out, void* stream) {
  WSIS_REQUIRE(M >= 0 && C >= 1 && d_out && (M == 0 || (d_mean && d_var)), "bad args");
  hipLaunchKernelGGL(bn_sync_pack_kernel, dim3(bn_sync_grid(C)), dim3(BN_SYNC_THREADS), 0, as_stream(stream), d_mean, d_var,
                     M, (int)C, d_out);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_bn_sync_combine(const double* d_gathered, int32_t R, int32_t C, float* d_mean, float* d_var,
                         float* d_running_mean, float* d_running_var, float momentum, double* d_count, void* stream) {
  WSIS_REQUIRE(R >= 1 && C >= 1 && d_gathered && d_mean && d_var && d_count, "bad args");
  WSIS_REQUIRE((d_running_mean == nullptr) == (d_running_var == nullptr), "running stats come in pairs");
  hipLaunchKernelGGL(bn_sync_combine_kernel, dim3(bn_sync_grid(C)), dim3(BN_SYNC_THREADS), 0, as_stream(stream), d_gathered,
                     (int)R, (int)C, d_mean, d_var, d_running_mean, d_running_var, momentum, d_count);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_bn_sync_sums_pack(const float* d_dgamma, const float* d_dbeta, int32_t C, double* d_out, void* stream) {
  WSIS_REQUIRE(C >= 1 && d_out, "bad args");
  hipLaunchKernelGGL(bn_sync_sums_pack_kernel, dim3(bn_sync_grid(C)), dim3(BN_SYNC_THREADS), 0, as_stream(stream), d_dgamma,
                     d_dbeta, (int)C, d_out);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_bn_sync_sums_scale(const double* d_sums, int64_t M, const double* d_count, int32_t C, float* d_sum_dz_xhat,
                            float* d_sum_dz, void* stream) {
  WSIS_REQUIRE(M >= 0 && C >= 1 && d_sums && d_count && d_sum_dz_xhat && d_sum_dz, "bad args");
  hipLaunchKernelGGL(bn_sync_sums_scale_kernel, dim3(bn_sync_grid(C)), dim3(BN_SYNC_THREADS), 0, as_stream(stream), d_sums, M,
                     d_count, (int)C, d_sum_dz_xhat, d_sum_dz);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_sync_bytes(void) { return (int64_t)kSyncSlotsTotal * (int64_t)sizeof(SyncSlot); }

int64_t wsis_colsum_workspace_bytes(int64_t M, int32_t C) {
  if (M < 0 || C < 4) return -1;
  int64_t per, G;
  colsum_plan(M, &per, &G);
  return (G > 1 ? G : 1) * (int64_t)C * (int64_t)sizeof(float) + 256;
}

int wsis_colsum(const float* d_x, int64_t M, int32_t C, float* d_out, void* d_ws, int64_t ws_bytes, void* d_sync,
                void* stream) {
  WSIS_REQUIRE(M >= 0 && C >= 4 && C % 4 == 0 && C <= 1024 && d_out, "colsum: C must be a multiple of 4, <= 1024");
  hipStream_t st = as_stream(stream);
  if (M == 0) {
    WSIS_HIP_CHECK(hipMemsetAsync(d_out, 0, sizeof(float) * (size_t)C, st));
    return WSIS_OK;
  }
  WSIS_REQUIRE(d_x && bn_aligned16({d_x, d_out}), "colsum: 16-byte alignment");
  int64_t per, G;
  colsum_plan(M, &per, &G);
  float* chunk = nullptr;
  unsigned* ticket = nullptr;
  if (G > 1) {
    WSIS_REQUIRE(d_ws && ws_bytes >= wsis_colsum_workspace_bytes(M, C), "workspace too small");
    chunk = static_cast<float*>(bn_align256(d_ws));
    WSIS_REQUIRE(d_sync, "colsum over more than one chunk needs a sync slot");
    ticket = static_cast<SyncSlot*>(d_sync)->ticket;
  }
  hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)G), dim3(256), 0, st, d_x, M, (int)C, per, chunk, d_out, ticket);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
