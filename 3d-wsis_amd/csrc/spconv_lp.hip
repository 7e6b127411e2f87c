// 16-bit sparse convolutions (bf16 / fp16 operands, fp32 accumulation) on the gfx950 matrix cores:
//
//   forward / dIn : out[r, :] = sum_k X[nbr[k][r], :] @ W[k] (+ bias + residual)   X, WT, residual 16-bit, out 16-bit
//                   (rounded once, at the end)
//   weight grad   : dW[k]     = sum_r X[nbr[k][r], :]^T (x) dY[r, :]  X, dY 16-bit, dW fp32
//
// Forward / dIn: one wave owns 32 rows of the tile order x NT * 32 output channels.  With the 32x32x16 lane map lane l
// (r = l & 31, h = l >> 5) holds A[row r][k = 8h + j] = X[src_r][c0 + 8h + j] -- one 16-byte load of its gathered row,
// straight into the A fragment -- and B[k = 8h + j][col r] = WT[k][co0 + r][c0 + 8h + j], 16 contiguous bytes of the
// B^T weights: no transpose, no LDS.  Every output element sums offset by offset, channel step by channel step, into
// its fp32 accumulator: the order of additions depends on the offset index only (bit-reproducible).  An offset that no
// row of the wave's 32 uses is skipped (the tile order groups rows with equal offset sets).
//
// Weight gradient: both MFMA operands sum over ROWS, the strided dimension of X and dY.  A workgroup owns one offset and
// one chunk of rows; per 32-row block it stages the gathered X rows and the paired dY rows in LDS TRANSPOSED
// ([channel][row], written with 16-bit stores from 16-byte global loads), so that every fragment read is one aligned
// 16-byte ds_read.  Each chunk writes its partial [Cin, Cout] slab to the workspace and a second launch adds the slabs
// in chunk order (no atomics).  One chunk: the slab is dW itself.
#include <algorithm>

#include "common.h"

using namespace wsis;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int LP_WAVES = 4;        // waves per workgroup of the forward / dIn kernel (independent 32-row tiles)
constexpr int LP_MAX_C = 512;      // channel limit of the weight-gradient LDS stage
constexpr int DW_PAD = 40;         // LDS row of the transposed stage: 32 rows + 8 (80 bytes: 16-byte aligned reads)
constexpr int DW_TPW = 4;          // output tiles (32 x 32) per wave of the weight-gradient kernel
constexpr int DW_MAX_CHUNKS = 64;
constexpr int64_t DW_CHUNK_ROWS = 2048;            // at least this many rows per chunk
constexpr int64_t DW_WS_CAP = (int64_t)256 << 20;  // the slabs of one product stay below this

__device__ __forceinline__ f32x16 mma(s16x8 a, s16x8 b, f32x16 c, __bf16) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                 0);
}
__device__ __forceinline__ f32x16 mma(s16x8 a, s16x8 b, f32x16 c, _Float16) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ s16x8 ld16(const void* p) { return *reinterpret_cast<const s16x8*>(p); }

template <typename T, int NT, int S>
__device__ __forceinline__ void chan_step(const T* xa, const T* wb, bool have, int c0, int Cin, f32x16 (&acc)[NT]) {
  s16x8 a[S], b[NT][S];
#pragma unroll
  for (int s = 0; s < S; ++s) a[s] = have ? ld16(xa + c0 + 16 * s) : s16x8{};
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int s = 0; s < S; ++s) b[n][s] = ld16(wb + (int64_t)n * 32 * Cin + c0 + 16 * s);
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int s = 0; s < S; ++s) acc[n] = mma(a[s], b[n][s], acc[n], T{});
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void spconv_lp_fwd_kernel(const T* __restrict__ X, const int32_t* __restrict__ nbr,
                                                            const int32_t* __restrict__ order, const T* __restrict__ WT,
                                                            int flip, const float* __restrict__ bias,
                                                            const T* __restrict__ res, T* __restrict__ out,
                                                            int64_t M_out, int K, int Cin, int Cout, int ncg) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int cg = blockIdx.x % ncg;
  const int64_t t0 = ((int64_t)(blockIdx.x / ncg) * LP_WAVES + (threadIdx.x >> 6)) * 32;
  if (t0 >= M_out) return;
  const int64_t t = t0 + r;
  const bool live = t < M_out;
  const int co0 = cg * NT * 32;
  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x16{};
  // the table entry of the next offset is loaded while the current one computes
  int nxt = !live ? -1 : (nbr ? nbr[t] : (int)t);
  for (int k = 0; k < K; ++k) {
    const int src = nxt;
    if (k + 1 < K) nxt = !live ? -1 : (nbr ? nbr[(int64_t)(k + 1) * M_out + t] : (int)t);
    if (__ballot(src >= 0) == 0ull) continue;       // no row of this tile pairs through offset k
    const int kk = flip ? K - 1 - k : k;
    const T* xa = X + (int64_t)(src < 0 ? 0 : src) * Cin + 8 * h;
    const T* wb = WT + ((int64_t)kk * Cout + co0 + r) * Cin + 8 * h;
    // 64 channels per step (8 loads in flight per lane and NT), a 32-channel step for the rest
    int c0 = 0;
    for (; c0 + 64 <= Cin; c0 += 64) chan_step<T, NT, 4>(xa, wb, src >= 0, c0, Cin, acc);
    if (c0 < Cin) chan_step<T, NT, 2>(xa, wb, src >= 0, c0, Cin, acc);
  }
  // epilogue: register i of lane (r, h) is tile row (i & 3) + 8 (i >> 2) + 4h, column r.  acc + bias (+ the residual,
  // widened exactly) in fp32, then ONE rounding; without a residual nothing is added (bit-identical to the form without)
  const int64_t my_row = live ? (order ? (int64_t)order[t] : t) : -1;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = co0 + n * 32 + r;
    const float b = bias ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
      const int64_t orow = __shfl(my_row, row);
      if (orow >= 0) {
        float v = acc[n][i] + b;
        if (res) v += (float)res[orow * Cout + col];
        out[orow * Cout + col] = (T)v;
      }
    }
  }
}

// grid: x = tile group (up to waves * DW_TPW output tiles of 32 x 32), y = row chunk, z = offset
template <typename T>
__global__ __launch_bounds__(256) void spconv_lp_dw_kernel(const T* __restrict__ X, const int32_t* __restrict__ nbr,
                                                           const int32_t* __restrict__ order, const T* __restrict__ dY,
                                                           float* __restrict__ slab, int64_t M_out, int K, int Cin,
                                                           int Cout, int64_t rows_per_chunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* Xt = reinterpret_cast<T*>(smem);                 // [Cin][DW_PAD]
  T* Yt = Xt + (int64_t)Cin * DW_PAD;                 // [Cout][DW_PAD]
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int k = blockIdx.z;
  const int ntc = Cout / 32, ntiles = (Cin / 32) * ntc;
  const int tile0 = blockIdx.x * nw * DW_TPW + wave;
  const int64_t rb0 = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t rb1 = M_out < rb0 + rows_per_chunk ? M_out : rb0 + rows_per_chunk;
  const int32_t* nk = nbr ? nbr + (int64_t)k * M_out : nullptr;
  f32x16 acc[DW_TPW];
#pragma unroll
  for (int j = 0; j < DW_TPW; ++j) acc[j] = f32x16{};
  const int xu = 32 * (Cin / 8), yu = 32 * (Cout / 8);
  for (int64_t rb = rb0; rb < rb1; rb += 32) {
    // stage: unit u = (8-channel group u >> 5, row u & 31); consecutive threads write consecutive LDS halves
    int active = 0;
    for (int u = threadIdx.x; u < xu + yu; u += blockDim.x) {
      const bool isx = u < xu;
      const int v = isx ? u : u - xu;
      const int rr = v & 31, g = v >> 5;
      const int64_t tt = rb + rr;
      const int src = tt < rb1 ? (nk ? nk[tt] : (int)tt) : -1;
      s16x8 val = s16x8{};
      if (src >= 0) {
        if (isx) {
          val = ld16(X + (int64_t)src * Cin + 8 * g);
          active = 1;
        } else {
          const int64_t orow = order ? (int64_t)order[tt] : tt;
          val = ld16(dY + orow * Cout + 8 * g);
        }
      }
      short* dst = reinterpret_cast<short*>(isx ? Xt : Yt) + (8 * g) * DW_PAD + rr;
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j * DW_PAD] = val[j];
    }
    if (!__syncthreads_or(active)) continue;     // no pair of offset k in these 32 rows
#pragma unroll
    for (int j = 0; j < DW_TPW; ++j) {
      const int tile = tile0 + j * nw;
      if (tile < ntiles) {
        const int ci0 = (tile / ntc) * 32, co0 = (tile % ntc) * 32;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const s16x8 a = ld16(Xt + (ci0 + r) * DW_PAD + 16 * s + 8 * h);
          const s16x8 b = ld16(Yt + (co0 + r) * DW_PAD + 16 * s + 8 * h);
          acc[j] = mma(a, b, acc[j], T{});
        }
      }
    }
    __syncthreads();
  }
  float* dst = slab + ((int64_t)blockIdx.y * K + k) * Cin * Cout;
#pragma unroll
  for (int j = 0; j < DW_TPW; ++j) {
    const int tile = tile0 + j * nw;
    if (tile < ntiles) {
      const int ci0 = (tile / ntc) * 32, co0 = (tile % ntc) * 32;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ci = ci0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        dst[(int64_t)ci * Cout + co0 + r] = acc[j][i];
      }
    }
  }
}

// dW[e] = sum over chunks c = 0, 1, ... of slab[c][e], in that order
__global__ __launch_bounds__(256) void spconv_lp_dw_sum_kernel(const float* __restrict__ slab, float* __restrict__ dW,
                                                               int64_t n, int chunks) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    float s = slab[e];
    for (int c = 1; c < chunks; ++c) s += slab[(int64_t)c * n + e];
    dW[e] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void weight_cast_lp_kernel(const float* __restrict__ W, T* __restrict__ out, int K,
                                                             int Cin, int Cout, int transpose, int flip) {
  const int64_t total = (int64_t)K * Cin * Cout;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(e % Cout);
    const int64_t q = e / Cout;
    const int ci = (int)(q % Cin);
    const int k = (int)(q / Cin);
    const int kk = flip ? K - 1 - k : k;
    const int64_t o = transpose ? ((int64_t)kk * Cout + co) * Cin + ci : ((int64_t)kk * Cin + ci) * Cout + co;
    out[o] = (T)W[e];
  }
}

int dw_chunks(int64_t M_out, int K, int Cin, int Cout) {
  int64_t c = ceil_div(M_out, DW_CHUNK_ROWS);
  c = std::min<int64_t>(c, DW_MAX_CHUNKS);
  c = std::min<int64_t>(c, std::max<int64_t>(1, DW_WS_CAP / ((int64_t)K * Cin * Cout * 4)));
  return (int)std::max<int64_t>(c, 1);
}

// the launch plan of both products for a shape: what the launches below run and wsis_spconv_lp_plan reports
struct LpPlan {
  int nt, ncg;             // forward / dIn: output tiles of 32 channels per wave, channel groups (grid = blocks)
  int64_t fwd_blocks;
  int chunks;              // weight gradient: row chunks (partial slabs), rows per chunk (a multiple of 32)
  int64_t rows_per_chunk;
  int nw, groups;          // waves per workgroup, tile groups (grid x)
  int64_t lds;             // dynamic LDS bytes of the transposed stage
};

LpPlan lp_plan(int64_t M_out, int K, int Cin, int Cout) {
  LpPlan p;
  // output channels per wave: two tiles where they split evenly and the level has rows enough to fill the CUs
  p.nt = (Cout / 32) % 2 == 0 && ceil_div(M_out, 32) * (Cout / 64) >= 4096 ? 2 : 1;
  p.ncg = Cout / (32 * p.nt);
  p.fwd_blocks = ceil_div(ceil_div(M_out, 32), LP_WAVES) * p.ncg;
  p.chunks = dw_chunks(M_out, K, Cin, Cout);
  p.rows_per_chunk = ceil_div(ceil_div(M_out, p.chunks), 32) * 32;
  const int ntiles = (Cin / 32) * (Cout / 32);
  p.nw = std::min(LP_WAVES, ntiles);
  p.groups = (int)ceil_div(ntiles, p.nw * DW_TPW);
  p.lds = (int64_t)(Cin + Cout) * DW_PAD * 2;
  return p;
}

template <typename T, int NT>
void launch_fwd(const void* X, const int32_t* nbr, const int32_t* order, const void* WT, int flip, const float* bias,
                const void* res, void* out, int64_t M_out, int K, int Cin, int Cout, const LpPlan& p, hipStream_t st) {
  hipLaunchKernelGGL((spconv_lp_fwd_kernel<T, NT>), dim3((unsigned)p.fwd_blocks), dim3(64 * LP_WAVES), 0, st,
                     static_cast<const T*>(X), nbr, order, static_cast<const T*>(WT), flip, bias,
                     static_cast<const T*>(res), static_cast<T*>(out), M_out, K, Cin, Cout, p.ncg);
}

template <typename T>
void launch_fwd_t(const void* X, const int32_t* nbr, const int32_t* order, const void* WT, int flip, const float* bias,
                  const void* res, void* out, int64_t M_out, int K, int Cin, int Cout, hipStream_t st) {
  const LpPlan p = lp_plan(M_out, K, Cin, Cout);
  if (p.nt == 2)
    launch_fwd<T, 2>(X, nbr, order, WT, flip, bias, res, out, M_out, K, Cin, Cout, p, st);
  else
    launch_fwd<T, 1>(X, nbr, order, WT, flip, bias, res, out, M_out, K, Cin, Cout, p, st);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int32_t wsis_spconv_lp_supported(int32_t K, int32_t Cin, int32_t Cout) {
  return (K >= 1 && Cin >= 32 && Cout >= 32 && Cin % 32 == 0 && Cout % 32 == 0 && Cin <= LP_MAX_C && Cout <= LP_MAX_C)
             ? 1
             : 0;
}

int32_t wsis_spconv_lp_plan(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, int32_t* out) {
  WSIS_REQUIRE(out, "null pointer");
  WSIS_REQUIRE(M_out >= 1 && M_out < (int64_t)1 << 31, "M_out must be in [1, 2^31)");
  WSIS_REQUIRE(wsis_spconv_lp_supported(K, Cin, Cout), "needs channel counts that are multiples of 32, at most 512");
  const LpPlan p = lp_plan(M_out, K, Cin, Cout);
  const int64_t v[8] = {p.nt, p.ncg, p.fwd_blocks, p.chunks, p.rows_per_chunk, p.nw, p.groups, p.lds};
  for (int i = 0; i < 8; ++i) WSIS_REQUIRE(v[i] <= INT32_MAX, "a plan value exceeds int32");
  for (int i = 0; i < 8; ++i) out[i] = (int32_t)v[i];
  return WSIS_OK;
}

int64_t wsis_spconv_fwd_lp_workspace_bytes(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout) {
  if (M_out < 0 || K < 1 || Cin < 1 || Cout < 1) return -1;
  return 256;
}

int wsis_spconv_fwd_lp(const void* d_X, const int32_t* d_nbr, const int32_t* d_order, const void* d_WT, int32_t flip,
                       const float* d_bias, void* d_out, int64_t M_in, int64_t M_out, int32_t K, int32_t Cin,
                       int32_t Cout, int32_t dtype, void* d_ws, int64_t ws_bytes, void* stream) {
  return wsis_spconv_fwd_lp_res(d_X, d_nbr, d_order, d_WT, flip, d_bias, nullptr, d_out, M_in, M_out, K, Cin, Cout, dtype,
                                d_ws, ws_bytes, stream);
}

int wsis_spconv_fwd_lp_res(const void* d_X, const int32_t* d_nbr, const int32_t* d_order, const void* d_WT,
                           int32_t flip, const float* d_bias, const void* d_residual, void* d_out, int64_t M_in,
                           int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* d_ws,
                           int64_t ws_bytes, void* stream) {
  (void)d_ws;
  (void)ws_bytes;
  WSIS_REQUIRE(M_in >= 0 && M_out >= 0, "bad sizes");
  WSIS_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (bf16) or 1 (fp16)");
  WSIS_REQUIRE(wsis_spconv_lp_supported(K, Cin, Cout), "needs channel counts that are multiples of 32, at most 512");
  if (M_out == 0) return WSIS_OK;
  WSIS_REQUIRE(d_WT && d_out && (d_X || M_in == 0), "null pointer");
  WSIS_REQUIRE(d_nbr || (K == 1 && M_in == M_out), "nbr may be null only for the dense 1x1 case");
  WSIS_REQUIRE(M_out < (int64_t)1 << 31 && M_in < (int64_t)1 << 31, "row count exceeds int32");
  WSIS_REQUIRE(M_in * Cin * 2 < (int64_t)1 << 31, "input tensor of 2 GiB or more (32-bit gather offsets)");
  WSIS_REQUIRE(aligned16(d_X) && aligned16(d_WT), "X and WT must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  if (dtype == 0)
    launch_fwd_t<__bf16>(d_X, d_nbr, d_order, d_WT, flip, d_bias, d_residual, d_out, M_out, K, Cin, Cout, st);
  else
    launch_fwd_t<_Float16>(d_X, d_nbr, d_order, d_WT, flip, d_bias, d_residual, d_out, M_out, K, Cin, Cout, st);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_spconv_dw_lp_workspace_bytes(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout) {
  if (M_out < 0 || K < 1 || Cin < 1 || Cout < 1) return -1;
  const int c = dw_chunks(M_out, K, Cin, Cout);
  return (c > 1 ? (int64_t)c * K * Cin * Cout * 4 : 0) + 256;
}

int wsis_spconv_dw_lp(const void* d_X, const int32_t* d_nbr, const int32_t* d_order, const void* d_dY, float* d_dW,
                      int64_t M_in, int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* d_ws,
                      int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(M_in >= 0 && M_out >= 0, "bad sizes");
  WSIS_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (bf16) or 1 (fp16)");
  WSIS_REQUIRE(wsis_spconv_lp_supported(K, Cin, Cout), "needs channel counts that are multiples of 32, at most 512");
  WSIS_REQUIRE(d_dW, "null pointer");
  hipStream_t st = as_stream(stream);
  const int64_t n = (int64_t)K * Cin * Cout;
  if (M_out == 0) {
    WSIS_HIP_CHECK(hipMemsetAsync(d_dW, 0, n * sizeof(float), st));
    return WSIS_OK;
  }
  WSIS_REQUIRE(d_dY && (d_X || M_in == 0), "null pointer");
  WSIS_REQUIRE(d_nbr || (K == 1 && M_in == M_out), "nbr may be null only for the dense 1x1 case");
  WSIS_REQUIRE(M_out < (int64_t)1 << 31 && M_in < (int64_t)1 << 31, "row count exceeds int32");
  WSIS_REQUIRE(M_in * Cin * 2 < (int64_t)1 << 31, "input tensor of 2 GiB or more (32-bit gather offsets)");
  WSIS_REQUIRE(aligned16(d_X) && aligned16(d_dY), "X and dY must be 16-byte aligned");
  const LpPlan p = lp_plan(M_out, K, Cin, Cout);
  WSIS_REQUIRE(ws_bytes >= wsis_spconv_dw_lp_workspace_bytes(M_out, K, Cin, Cout) && (p.chunks == 1 || d_ws),
               "workspace too small");
  float* slab = p.chunks > 1 ? static_cast<float*>(d_ws) : d_dW;
  const dim3 grid(p.groups, p.chunks, K);
  if (dtype == 0)
    hipLaunchKernelGGL(spconv_lp_dw_kernel<__bf16>, grid, dim3(64 * p.nw), (size_t)p.lds, st,
                       static_cast<const __bf16*>(d_X), d_nbr, d_order, static_cast<const __bf16*>(d_dY), slab, M_out,
                       K, Cin, Cout, p.rows_per_chunk);
  else
    hipLaunchKernelGGL(spconv_lp_dw_kernel<_Float16>, grid, dim3(64 * p.nw), (size_t)p.lds, st,
                       static_cast<const _Float16*>(d_X), d_nbr, d_order, static_cast<const _Float16*>(d_dY), slab,
                       M_out, K, Cin, Cout, p.rows_per_chunk);
  WSIS_LAUNCH_CHECK();
  if (p.chunks > 1) {
    hipLaunchKernelGGL(spconv_lp_dw_sum_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, slab, d_dW, n, p.chunks);
    WSIS_LAUNCH_CHECK();
  }
  return WSIS_OK;
}

int wsis_weight_cast_lp(const float* d_W, void* d_out, int32_t K, int32_t Cin, int32_t Cout, int32_t transpose,
                        int32_t flip, int32_t dtype, void* stream) {
  WSIS_REQUIRE(K >= 1 && Cin >= 1 && Cout >= 1 && d_W && d_out, "bad args");
  WSIS_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (bf16) or 1 (fp16)");
  const int64_t total = (int64_t)K * Cin * Cout;
  hipStream_t st = as_stream(stream);
  if (dtype == 0)
    hipLaunchKernelGGL(weight_cast_lp_kernel<__bf16>, dim3(grid_for(total, 256)), dim3(256), 0, st, d_W,
                       static_cast<__bf16*>(d_out), K, Cin, Cout, transpose, flip);
  else
    hipLaunchKernelGGL(weight_cast_lp_kernel<_Float16>, dim3(grid_for(total, 256)), dim3(256), 0, st, d_W,
                       static_cast<_Float16*>(d_out), K, Cin, Cout, transpose, flip);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}
