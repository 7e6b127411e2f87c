// LSTMCellEx of the superpoint GNN: LSTM cell with an input gate and per-row normalisation of the gate
// pre-activations (modules/model/spg_modules.py:264-318), the cell of the 'lstm_R_...' configurations
// (modules/model/graphnet.py:77-92).  Organised as gru.hip: one kernel forward, one backward (+ a fixed-order reduce of
// the parameter gradients), one wavefront per row, the weights resident in LDS, C = H = 32.
//
//   xin = sigmoid(Wig h + big) * x
//   gi = rownorm(Wih xin + bih), gh = rownorm(Whh h + bhh)    rownorm(v) = (v - mean)/sqrt(var + 1e-5) over 4C; unlike
//                                                             the GRU cell the biases are INSIDE the norm
//   (i, f, g, o) = chunk4(gi + gh);  i, f, o = sigmoid, g = tanh
//   cy = f * c + i * g,  hy = o * tanh(cy)
//
// The 4C = 128 gate values of a row sit two per lane: lane l holds o = l and o = l + 64, so lane c < 32 holds (i_c, g_c)
// and lane 32 + c holds (f_c, o_c); one xor-32 exchange gives every lane the four gates of channel c = l & 31.
//
// LDS: the forward reads a weight row per lane (W[o = lane][j]), the backward a weight column per lane (W[o][j = c]).
// ONE image with rows padded to 33 floats serves both: address o * 33 + j puts the 32 lanes of a half-wave on 32
// different banks whether o or j runs with the lane -- 38 KB of weights instead of the 70 KB of two orientations.
#include <algorithm>

#include "common.h"

using namespace wsis;

namespace {

constexpr int LC = 32;             // channels
constexpr int L4 = 128;            // 4 * channels
constexpr int LSTM_WF = 8;         // forward: rows (= waves) per weight staging
constexpr int LSTM_WAVES = 4;      // backward: waves per workgroup
constexpr int LSTM_ROWS = 3;       // backward: rows per wave -> LSTM_WAVES * LSTM_ROWS rows per workgroup, as the GRU cell
constexpr int LSTM_MAX_WG = 256;   // one workgroup per CU at most; beyond it the waves stride over the rows
constexpr int LSTM_P = 2 * L4 * LC + LC * LC + 2 * L4 + LC;   // parameter-gradient floats: Wih, Whh, Wig, bih, bhh, big
constexpr int LP = LC + 1;         // padded row of a weight image

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }

struct LstmLds {
  float Wih[L4][LP];               // [o][j]
  float Whh[L4][LP];
  float Wig[LC][LP];               // [c][j]
  float vec[LSTM_WF][2][LC];       // per-wave h row and xin row (LSTM_WF >= LSTM_WAVES)
  float dg[LSTM_WAVES][2][L4];     // per-wave d gi, d gh (backward)
};
static_assert(sizeof(float) * LSTM_P <= sizeof(float) * (2 * L4 * LP + LC * LP), "the slab reuses the weight images");
static_assert(LSTM_WF >= LSTM_WAVES, "per-wave rows");

// the three weight matrices -> LDS.  Every global load of the workgroup is issued before the first LDS store: one
// memory latency for the whole staging.  The four scalar stores of a float4 go to banks (o + j + e) % 32: the 32 lanes
// of a half-wave cover 4 values of o and 8 of j = 4k, all different
template <int NT>
__device__ __forceinline__ void lstm_load_weights(LstmLds& L, const float* Wig, const float* Wih, const float* Whh) {
  constexpr int N_IH = (L4 * LC / 4 + NT - 1) / NT;      // float4 pieces per thread of Wih / Whh
  constexpr int N_IG = (LC * LC / 4 + NT - 1) / NT;
  float4 a[N_IH], b[N_IH], g[N_IG];
#pragma unroll
  for (int u = 0; u < N_IH; ++u) {
    const int f4 = threadIdx.x + u * NT;
    const bool ok = f4 < L4 * LC / 4;
    a[u] = ok ? reinterpret_cast<const float4*>(Wih)[f4] : make_float4(0.f, 0.f, 0.f, 0.f);
    b[u] = ok ? reinterpret_cast<const float4*>(Whh)[f4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int u = 0; u < N_IG; ++u) {
    const int f4 = threadIdx.x + u * NT;
    g[u] = f4 < LC * LC / 4 ? reinterpret_cast<const float4*>(Wig)[f4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int u = 0; u < N_IH; ++u) {
    const int f4 = threadIdx.x + u * NT;
    if (f4 < L4 * LC / 4) {
      const int o = (f4 * 4) / LC, j = (f4 * 4) % LC;
      const float av[4] = {a[u].x, a[u].y, a[u].z, a[u].w}, bv[4] = {b[u].x, b[u].y, b[u].z, b[u].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        L.Wih[o][j + e] = av[e];
        L.Whh[o][j + e] = bv[e];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < N_IG; ++u) {
    const int f4 = threadIdx.x + u * NT;
    if (f4 < LC * LC / 4) {
      const int c = (f4 * 4) / LC, j = (f4 * 4) % LC;
      const float gv[4] = {g[u].x, g[u].y, g[u].z, g[u].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) L.Wig[c][j + e] = gv[e];
    }
  }
}

// forward of one row by one wave; what the backward needs stays in registers.  c = lane & 31 on every lane
struct LstmRow {
  float x, h, c0;      // inputs of channel c (both half-waves hold them)
  float gin, xin;      // input gate and gated input of channel c
  float gi1, gi2;      // normalised gi[o = lane], gi[o = lane + 64]
  float gh1, gh2;
  float sig_i, sig_h;  // 1/sqrt(var + eps) of the two row norms
  float i, f, g, o;    // the gates of channel c
  float tc;            // tanh(cy)
  float cy, hy;
};

__device__ __forceinline__ LstmRow lstm_row_fwd(LstmLds& L, int wave, int lane, const float* __restrict__ x,
                                                const float* __restrict__ h, const float* __restrict__ c0,
                                                const float* __restrict__ big, const float* __restrict__ bih,
                                                const float* __restrict__ bhh, int64_t row) {
  LstmRow R;
  const int c = lane & 31;
  R.x = x[row * LC + c];
  R.h = h[row * LC + c];
  R.c0 = c0[row * LC + c];
  float* hrow = L.vec[wave][0];
  float* xrow = L.vec[wave][1];
  if (lane < 32) hrow[c] = R.h;
  // input gate
  float a = big[c];
#pragma unroll
  for (int j = 0; j < LC; ++j) a += L.Wig[c][j] * hrow[j];
  R.gin = sigm(a);
  R.xin = R.gin * R.x;
  if (lane < 32) xrow[c] = R.xin;
  // gi = Wih xin + bih, gh = Whh h + bhh at o = lane and o = lane + 64
  float gi1 = bih[lane], gi2 = bih[lane + 64], gh1 = bhh[lane], gh2 = bhh[lane + 64];
#pragma unroll
  for (int j = 0; j < LC; ++j) {
    const float xv = xrow[j], hv = hrow[j];
    gi1 += L.Wih[lane][j] * xv;
    gh1 += L.Whh[lane][j] * hv;
    gi2 += L.Wih[lane + 64][j] * xv;
    gh2 += L.Whh[lane + 64][j] * hv;
  }
  // row norms over the 128 values
  const float inv = 1.0f / (float)L4;
  const float mi = wsum(gi1 + gi2) * inv;
  const float mh = wsum(gh1 + gh2) * inv;
  const float di1 = gi1 - mi, di2 = gi2 - mi, dh1 = gh1 - mh, dh2 = gh2 - mh;
  const float vi = wsum(di1 * di1 + di2 * di2) * inv;
  const float vh = wsum(dh1 * dh1 + dh2 * dh2) * inv;
  R.sig_i = 1.0f / sqrtf(vi + 1e-5f);
  R.sig_h = 1.0f / sqrtf(vh + 1e-5f);
  R.gi1 = di1 * R.sig_i;
  R.gi2 = di2 * R.sig_i;
  R.gh1 = dh1 * R.sig_h;
  R.gh2 = dh2 * R.sig_h;
  // lane c: (i, g); lane 32 + c: (f, o).  Every lane activates its own two and fetches the other two
  const bool lo = lane < 32;
  const float p1 = R.gi1 + R.gh1, p2 = R.gi2 + R.gh2;
  const float a1 = sigm(p1);                       // i or f
  const float a2 = lo ? tanhf(p2) : sigm(p2);      // g or o
  const float b1 = __shfl_xor(a1, 32, 64), b2 = __shfl_xor(a2, 32, 64);
  R.i = lo ? a1 : b1;
  R.f = lo ? b1 : a1;
  R.g = lo ? a2 : b2;
  R.o = lo ? b2 : a2;
  R.cy = R.f * R.c0 + R.i * R.g;
  R.tc = tanhf(R.cy);
  R.hy = R.o * R.tc;
  return R;
}

__global__ __launch_bounds__(64 * LSTM_WF) void lstm_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ c0,
    const float* __restrict__ Wig, const float* __restrict__ big, const float* __restrict__ Wih,
    const float* __restrict__ Whh, const float* __restrict__ bih, const float* __restrict__ bhh,
    float* __restrict__ hy, float* __restrict__ cy, int64_t S) {
  __shared__ LstmLds L;
  lstm_load_weights<64 * LSTM_WF>(L, Wig, Wih, Whh);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nw = (int64_t)gridDim.x * LSTM_WF;
  for (int64_t row = (int64_t)blockIdx.x * LSTM_WF + wave; row < S; row += nw) {
    const LstmRow R = lstm_row_fwd(L, wave, lane, x, h, c0, big, bih, bhh, row);
    if (lane < 32) {
      hy[row * LC + lane] = R.hy;
      cy[row * LC + lane] = R.cy;
    }
  }
}

// backward: recomputes the row forward, then the gradients; parameter gradients accumulate in registers over the
// wave's rows, the four waves merge them in wave order in LDS and the workgroup's slab goes to partial[block][LSTM_P]
__global__ __launch_bounds__(64 * LSTM_WAVES) void lstm_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ c0,
    const float* __restrict__ Wig, const float* __restrict__ big, const float* __restrict__ Wih,
    const float* __restrict__ Whh, const float* __restrict__ bih, const float* __restrict__ bhh,
    const float* __restrict__ dhy, const float* __restrict__ dcy, float* __restrict__ dx, float* __restrict__ dh,
    float* __restrict__ dc, float* __restrict__ partial, int64_t S) {
  __shared__ LstmLds L;
  lstm_load_weights<64 * LSTM_WAVES>(L, Wig, Wih, Whh);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, hi = lane >> 5;
  const bool lo = lane < 32;
  const int64_t nw = (int64_t)gridDim.x * LSTM_WAVES;
  // parameter-gradient accumulators: lane owns column j = c and rows o = hi + 2t
  float aWih[L4 / 2], aWhh[L4 / 2], aWig[LC / 2];
#pragma unroll
  for (int t = 0; t < L4 / 2; ++t) aWih[t] = aWhh[t] = 0.f;
#pragma unroll
  for (int t = 0; t < LC / 2; ++t) aWig[t] = 0.f;
  float abih1 = 0.f, abih2 = 0.f, abhh1 = 0.f, abhh2 = 0.f, abig = 0.f;   // biases at o = lane, o = lane + 64, c
  float* dgi = L.dg[wave][0];
  float* dgh = L.dg[wave][1];
  for (int64_t row = (int64_t)blockIdx.x * LSTM_WAVES + wave; row < S; row += nw) {
    const LstmRow R = lstm_row_fwd(L, wave, lane, x, h, c0, big, bih, bhh, row);
    const float ghy = dhy ? dhy[row * LC + c] : 0.0f;      // (either upstream gradient may be absent = zero)
    const float gcy = dcy ? dcy[row * LC + c] : 0.0f;
    // hy = o * tanh(cy), cy = f * c + i * g
    const float dcy_t = gcy + ghy * R.o * (1.0f - R.tc * R.tc);
    const float dpi = dcy_t * R.g * R.i * (1.0f - R.i);
    const float dpf = dcy_t * R.c0 * R.f * (1.0f - R.f);
    const float dpg = dcy_t * R.i * (1.0f - R.g * R.g);
    const float dpo = ghy * R.tc * R.o * (1.0f - R.o);
    // the o-indexed layout of the pre-activations; gi + gh: both norms see the same upstream gradient
    const float y1 = lo ? dpi : dpf;
    const float y2 = lo ? dpg : dpo;
    // rownorm backward: dg = (dy - mean(dy) - yhat * mean(dy * yhat)) * sig
    const float inv = 1.0f / (float)L4;
    const float m1 = wsum(y1 + y2) * inv;
    const float m2i = wsum(y1 * R.gi1 + y2 * R.gi2) * inv;
    const float m2h = wsum(y1 * R.gh1 + y2 * R.gh2) * inv;
    const float dgi1 = (y1 - m1 - R.gi1 * m2i) * R.sig_i;
    const float dgi2 = (y2 - m1 - R.gi2 * m2i) * R.sig_i;
    const float dgh1 = (y1 - m1 - R.gh1 * m2h) * R.sig_h;
    const float dgh2 = (y2 - m1 - R.gh2 * m2h) * R.sig_h;
    abih1 += dgi1;                                         // the biases sit inside the norm
    abih2 += dgi2;
    abhh1 += dgh1;
    abhh2 += dgh2;
    dgi[lane] = dgi1;
    dgi[64 + lane] = dgi2;
    dgh[lane] = dgh1;
    dgh[64 + lane] = dgh2;
    // dxin[j] = sum_o Wih[o][j] dgi[o],  dh[j] = sum_o Whh[o][j] dgh[o]    (lane j = c; the half-waves split o)
    float dxin = 0.f, dhh = 0.f;
#pragma unroll     // fully: the accumulators must be indexed by constants to stay in registers
    for (int t = 0; t < L4 / 2; ++t) {
      const int o = hi + 2 * t;
      const float gi_o = dgi[o], gh_o = dgh[o];
      dxin += L.Wih[o][c] * gi_o;
      dhh += L.Whh[o][c] * gh_o;
      aWih[t] += gi_o * R.xin;       // dWih[o][j = c]
      aWhh[t] += gh_o * R.h;
    }
    dxin += __shfl_xor(dxin, 32, 64);
    dhh += __shfl_xor(dhh, 32, 64);
    // input gate: xin = gin * x
    const float dgpre = dxin * R.x * R.gin * (1.0f - R.gin);
    abig += dgpre;
    float* dgp = dgi;                 // reuse the scratch row for dgpre (all reads of dgi are done)
    if (lo) dgp[c] = dgpre;
    float dhg = 0.f;
#pragma unroll
    for (int t = 0; t < LC / 2; ++t) {
      const int cc = hi + 2 * t;      // rows of Wig handled by this half
      const float gp = dgp[cc];
      dhg += L.Wig[cc][c] * gp;       // dh[j = c] += Wig[cc][j] * dgpre[cc]
      aWig[t] += gp * R.h;            // dWig[cc][j = c]
    }
    dhg += __shfl_xor(dhg, 32, 64);
    if (lo) {
      dx[row * LC + c] = dxin * R.gin;
      dh[row * LC + c] = dhh + dhg;
      dc[row * LC + c] = dcy_t * R.f;
    }
  }
  // workgroup slab [Wih 128x32][Whh 128x32][Wig 32x32][bih 128][bhh 128][big 32] in the LDS of the weight images (no
  // longer needed): wave 0 stores its accumulators, waves 1..3 add theirs one after the other -- every element is owned
  // by the same lane in every wave, the order of the sum is the wave order -- and the sum goes out coalesced
  float* const slab = reinterpret_cast<float*>(&L);
  float* const pb = slab + 2 * L4 * LC + LC * LC;
  for (int w = 0; w < LSTM_WAVES; ++w) {
    __syncthreads();                 // (first pass: every wave is done with the weights)
    if (wave != w) continue;
    if (w == 0) {
#pragma unroll
      for (int t = 0; t < L4 / 2; ++t) {
        const int o = hi + 2 * t;
        slab[o * LC + c] = aWih[t];
        slab[L4 * LC + o * LC + c] = aWhh[t];
      }
#pragma unroll
      for (int t = 0; t < LC / 2; ++t) slab[2 * L4 * LC + (hi + 2 * t) * LC + c] = aWig[t];
      pb[lane] = abih1;
      pb[64 + lane] = abih2;
      pb[L4 + lane] = abhh1;
      pb[L4 + 64 + lane] = abhh2;
      if (lo) pb[2 * L4 + lane] = abig;
    } else {
#pragma unroll
      for (int t = 0; t < L4 / 2; ++t) {
        const int o = hi + 2 * t;
        slab[o * LC + c] += aWih[t];
        slab[L4 * LC + o * LC + c] += aWhh[t];
      }
#pragma unroll
      for (int t = 0; t < LC / 2; ++t) slab[2 * L4 * LC + (hi + 2 * t) * LC + c] += aWig[t];
      pb[lane] += abih1;
      pb[64 + lane] += abih2;
      pb[L4 + lane] += abhh1;
      pb[L4 + 64 + lane] += abhh2;
      if (lo) pb[2 * L4 + lane] += abig;
    }
  }
  __syncthreads();
  float* p = partial + (int64_t)blockIdx.x * LSTM_P;
  for (int f = threadIdx.x; f < LSTM_P; f += blockDim.x) p[f] = slab[f];
}

constexpr int RED_OUT = 32;    // outputs per workgroup of the slab reduce
constexpr int RED_LANES = 8;   // slab lanes per output
constexpr int RED_DEPTH = 8;   // slabs in flight per lane

__global__ __launch_bounds__(RED_OUT * RED_LANES) void lstm_reduce_kernel(
    const float* __restrict__ partial, int nslab, float* __restrict__ dWih, float* __restrict__ dWhh,
    float* __restrict__ dWig, float* __restrict__ dbih, float* __restrict__ dbhh, float* __restrict__ dbig) {
  // 32 outputs x 8 slab lanes per workgroup: lane y sums slabs y, y+8, ... in order, then the 8 partial sums are
  // added in lane order -- a fixed summation tree, independent of the launch
  __shared__ float part[RED_LANES][RED_OUT];
  const int ox = threadIdx.x % RED_OUT, sy = threadIdx.x / RED_OUT;
  const int i = blockIdx.x * RED_OUT + ox;
  float s = 0.f;
  if (i < LSTM_P) {
    int k = sy;
    for (; k + (RED_DEPTH - 1) * RED_LANES < nslab; k += RED_DEPTH * RED_LANES) {      // loads first, added in the same order
      float t[RED_DEPTH];
#pragma unroll
      for (int j = 0; j < RED_DEPTH; ++j) t[j] = partial[(int64_t)(k + j * RED_LANES) * LSTM_P + i];
#pragma unroll
      for (int j = 0; j < RED_DEPTH; ++j) s += t[j];
    }
    for (; k < nslab; k += RED_LANES) s += partial[(int64_t)k * LSTM_P + i];
  }
  part[sy][ox] = s;
  __syncthreads();
  if (sy != 0 || i >= LSTM_P) return;
#pragma unroll
  for (int y = 1; y < RED_LANES; ++y) s += part[y][ox];
  constexpr int E_IH = L4 * LC, E_HH = 2 * L4 * LC, E_IG = E_HH + LC * LC, E_BIH = E_IG + L4, E_BHH = E_BIH + L4;
  if (i < E_IH)
    dWih[i] = s;
  else if (i < E_HH)
    dWhh[i - E_IH] = s;
  else if (i < E_IG)
    dWig[i - E_HH] = s;
  else if (i < E_BIH)
    dbih[i - E_IG] = s;
  else if (i < E_BHH)
    dbhh[i - E_BIH] = s;
  else
    dbig[i - E_BHH] = s;
}

int lstm_blocks(int64_t S, int rows_per_wg) {
  int64_t b = ceil_div(S, rows_per_wg);
  if (b < 1) b = 1;
  if (b > LSTM_MAX_WG) b = LSTM_MAX_WG;
  return (int)b;
}

}  // namespace

extern "C" {

int64_t wsis_lstm_cell_workspace_bytes(int64_t S) {
  if (S < 0) return -1;
  return (int64_t)lstm_blocks(S, LSTM_WAVES * LSTM_ROWS) * LSTM_P * (int64_t)sizeof(float) + 256;
}

int wsis_lstm_cell_fwd(const float* d_x, const float* d_h, const float* d_c, const float* d_Wig, const float* d_big,
                       const float* d_Wih, const float* d_Whh, const float* d_bih, const float* d_bhh, float* d_hy,
                       float* d_cy, int64_t S, int32_t C, void* stream) {
  WSIS_REQUIRE(S >= 0 && C == LC, "LSTMCellEx kernel supports C == 32");
  if (S == 0) return WSIS_OK;
  WSIS_REQUIRE(d_x && d_h && d_c && d_Wig && d_big && d_Wih && d_Whh && d_bih && d_bhh && d_hy && d_cy, "null pointer");
  hipLaunchKernelGGL(lstm_fwd_kernel, dim3(lstm_blocks(S, LSTM_WF)), dim3(64 * LSTM_WF), 0, as_stream(stream), d_x, d_h,
                     d_c, d_Wig, d_big, d_Wih, d_Whh, d_bih, d_bhh, d_hy, d_cy, S);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_lstm_cell_bwd(const float* d_x, const float* d_h, const float* d_c, const float* d_Wig, const float* d_big,
                       const float* d_Wih, const float* d_Whh, const float* d_bih, const float* d_bhh,
                       const float* d_dhy, const float* d_dcy, float* d_dx, float* d_dh, float* d_dc, float* d_dWig,
                       float* d_dbig, float* d_dWih, float* d_dWhh, float* d_dbih, float* d_dbhh, int64_t S, int32_t C,
                       void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(S >= 1 && C == LC, "LSTMCellEx kernel supports C == 32, S >= 1");
  WSIS_REQUIRE(d_x && d_h && d_c && d_Wig && d_big && d_Wih && d_Whh && d_bih && d_bhh && (d_dhy || d_dcy) && d_dx &&
                   d_dh && d_dc && d_dWig && d_dbig && d_dWih && d_dWhh && d_dbih && d_dbhh && d_ws,
               "null pointer");
  WSIS_REQUIRE(ws_bytes >= wsis_lstm_cell_workspace_bytes(S), "workspace too small");
  const int nb = lstm_blocks(S, LSTM_WAVES * LSTM_ROWS);
  float* partial = static_cast<float*>(d_ws);
  hipLaunchKernelGGL(lstm_bwd_kernel, dim3(nb), dim3(64 * LSTM_WAVES), 0, as_stream(stream), d_x, d_h, d_c, d_Wig, d_big,
                     d_Wih, d_Whh, d_bih, d_bhh, d_dhy, d_dcy, d_dx, d_dh, d_dc, partial, S);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(lstm_reduce_kernel, dim3((LSTM_P + RED_OUT - 1) / RED_OUT), dim3(RED_OUT * RED_LANES), 0,
                     as_stream(stream), partial, nb, d_dWih, d_dWhh, d_dWig, d_dbih, d_dbhh, d_dbig);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
