// Per-scene preparation of a training item on the device: ScanNetV2Inst_spg.__getitem__ of the reference
// (modules/datasets/scannetv2_dataset.py:96-190) and its S3DIS twin (s3dis_dataset.py:126-206), which the host class
// wsis_datasets.ScenePrep mirrors in numpy.
//
//   data_aug_with_graph, xyz * scale, its bounds             :194-209, :149-152     wsis_sp_affine
//   elastic :222-249 (PointGroup's distortion), blur / interpolation               wsis_elastic_blur / _apply
//   crop :252-273 / crop_v2 s3dis_dataset.py:285-319, one round                     wsis_sp_crop_mask
//   the five boolean-mask gathers and the dtypes of collate_fn :155-160, :176-181   wsis_sp_emit
//   np.unique(superpoint, return_inverse=True) :169, get_cropped_inst_label :311-330  wsis_sp_tables + wsis_sp_relabel
//   get_instance_info :275-309                                                      wsis_sp_instance_info
//
// The crop loops stay on the host (the order of the random draws is the contract); a round is one launch here and one
// count read back.  Everything per point after the last round is one pass per stage; the two id tables are O(ids).
//
// Reproducibility: no floating-point atomic.  Minima and maxima are integer atomics on the ORDERED bit pattern of a
// double (order-free, exact); counts are integer atomics; presence flags are plain stores of 1.  The instance sums are
// one wave per instance over its CSR row, lane l taking the points l, l + 64, ... in order, then one xor butterfly: a fixed
// order, but not numpy's row order (the mean may differ from the reference's in the last fp32 bit, never by more).
// The file is built with -ffp-contract=off; the one fused operation, the augmentation product, is an explicit fma:
// fma(z, m[2][j], fma(y, m[1][j], x * m[0][j])) is what np.matmul returns for an [N,3] x [3,3] fp64 product.
#include "common.h"

using namespace wsis;

namespace {

constexpr int SP_BLOCK = 256;
constexpr int SP_WAVES = SP_BLOCK / 64;
constexpr int SP_PER = 4;                        // consecutive points per thread of the mask-ordered passes
constexpr int SP_TILE = SP_BLOCK * SP_PER;       // points per workgroup there
constexpr int SP_SCAN_BLOCK = 1024;              // the one workgroup of the id tables
constexpr int EL_BLOCK = 256;                    // elastic: cells (blur pass) / points (apply) per workgroup
constexpr int64_t SP_NONE = -100;

// words of the state block (uint64 each)
constexpr int ST_MIN = 0, ST_MAX = 3, ST_BAD = 6, ST_LOCMAX = 8, ST_SNEW = 11, ST_KINST = 12, ST_ROUND0 = 16;

struct M9 {
  double m[9];
};
struct D3 {
  double v[3];
};
struct F3 {
  float v[3];
  int on;
};

// order-preserving map double -> uint64 (negative values: all bits flipped, others: the sign bit set)
__device__ __forceinline__ unsigned long long ordered_bits(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double wave_min(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double t = __shfl_xor(x, m);
    x = t < x ? t : x;
  }
  return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double t = __shfl_xor(x, m);
    x = t > x ? t : x;
  }
  return x;
}

__global__ void sp_state_init_kernel(unsigned long long* __restrict__ st) {
  const int i = threadIdx.x;
  if (i >= WSIS_SP_STATE_WORDS) return;
  unsigned long long v = 0ull;
  if (i < ST_MAX) v = ~0ull;                                       // running minima start at the largest key
  if (i >= ST_ROUND0 && ((i - ST_ROUND0) & 3) != 0) v = ~0ull;     // the kept-point minima of a round
  st[i] = v;
}

// ---- augmentation product, scaling, bounds
template <typename T>
__global__ __launch_bounds__(SP_BLOCK) void sp_affine_kernel(const T* __restrict__ in, const int64_t* __restrict__ pick,
                                                             int64_t n_src, int64_t n, M9 a, double scale,
                                                             double* __restrict__ middle, double* __restrict__ scaled,
                                                             unsigned long long* __restrict__ st) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  int bad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t p = pick ? pick[i] : i;
    if (p < 0 || p >= n_src) {
      p = 0;
      bad = 1;
    }
    const double x = (double)in[3 * p], y = (double)in[3 * p + 1], z = (double)in[3 * p + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double v = fma(z, a.m[6 + j], fma(y, a.m[3 + j], x * a.m[j]));
      middle[3 * i + j] = v;
      if (scaled) {
        const double s = v * scale;
        scaled[3 * i + j] = s;
        lo[j] = s < lo[j] ? s : lo[j];
        hi[j] = s > hi[j] ? s : hi[j];
      }
    }
  }
  if (!st) return;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double l = wave_min(lo[j]), h = wave_max(hi[j]);
    if (lane == 0 && scaled && l <= h) {
      atomicMin(st + ST_MIN + j, ordered_bits(l));
      atomicMax(st + ST_MAX + j, ordered_bits(h));
    }
  }
  const unsigned long long b = __ballot(bad);
  if (lane == 0 && b) atomicAdd(st + ST_BAD, (unsigned long long)__popcll(b));
}

// ---- elastic :222-249.  The three noise grids are blurred by six passes of the 3-tap box filter (scipy.ndimage.convolve,
// mode="constant", cval=0: the sum in fp64 in tap order from 0.0, one rounding to fp32 per pass), then every point is
// displaced by the trilinear interpolation of the grids (scipy's RegularGridInterpolator, fill_value 0).  All of it is
// fp64 in the written order; with -ffp-contract=off and the correctly rounded fp64 division the result is scipy's bit
// for bit.
__global__ __launch_bounds__(EL_BLOCK) void sp_elastic_blur_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                   int64_t cells, int64_t stride, int len) {
  const int64_t i = (int64_t)blockIdx.x * EL_BLOCK + threadIdx.x;
  if (i >= cells) return;
  const double w = (double)(1.0f / 3.0f);
  const float* g = in + (int64_t)blockIdx.y * cells;             // blockIdx.y: one of the three grids
  const int64_t k = (i / stride) % len;                          // the cell's coordinate along the pass's axis
  const double l = k > 0 ? (double)g[i - stride] : 0.0;
  const double c = (double)g[i];
  const double r = k < len - 1 ? (double)g[i + stride] : 0.0;
  out[(int64_t)blockIdx.y * cells + i] = (float)((w * l + w * c) + w * r);
}

struct I3 {
  int v[3];
};

// node k of axis j is first.v[j] + step * k (exact integers); one thread per point
__global__ __launch_bounds__(EL_BLOCK) void sp_elastic_apply_kernel(double* __restrict__ xyz, int64_t n,
                                                                    const float* __restrict__ grids, I3 bb, D3 first,
                                                                    double step, double mag,
                                                                    unsigned long long* __restrict__ bounds) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  const int64_t p = (int64_t)blockIdx.x * EL_BLOCK + threadIdx.x;
  if (p < n) {
    double x[3], t[3], d[3] = {0.0, 0.0, 0.0};
    int64_t idx[3];
    bool inside = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      x[j] = xyz[3 * p + j];
      inside = inside && x[j] >= first.v[j] && x[j] <= first.v[j] + step * (double)(bb.v[j] - 1);
    }
    if (inside) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        // c = number of nodes < x (np.searchsorted, side left): an estimate, then exact compares against the nodes
        int64_t c = (int64_t)((x[j] - first.v[j]) / step) + 1;
        c = c < 0 ? 0 : (c > bb.v[j] ? bb.v[j] : c);
        while (c > 0 && first.v[j] + step * (double)(c - 1) >= x[j]) --c;
        while (c < bb.v[j] && first.v[j] + step * (double)c < x[j]) ++c;
        int64_t i = c - 1;
        i = i < 0 ? 0 : (i > bb.v[j] - 2 ? bb.v[j] - 2 : i);
        const double a = first.v[j] + step * (double)i, b = first.v[j] + step * (double)(i + 1);
        idx[j] = i;
        t[j] = (x[j] - a) / (b - a);
      }
      const int64_t s1 = bb.v[2], s0 = (int64_t)bb.v[1] * bb.v[2], cells = s0 * bb.v[0];
      const int64_t base = (idx[0] * bb.v[1] + idx[1]) * bb.v[2] + idx[2];
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) {
        const int cx = (corner >> 2) & 1, cy = (corner >> 1) & 1, cz = corner & 1;
        const double w = ((cx ? t[0] : 1.0 - t[0]) * (cy ? t[1] : 1.0 - t[1])) * (cz ? t[2] : 1.0 - t[2]);
        const int64_t o = base + cx * s0 + cy * s1 + cz;
#pragma unroll
        for (int m = 0; m < 3; ++m) d[m] += (double)grids[m * cells + o] * w;
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double v = x[j] + d[j] * mag;
      xyz[3 * p + j] = v;
      lo[j] = v;
      hi[j] = v;
    }
  }
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double l = wave_min(lo[j]), h = wave_max(hi[j]);
    if (lane == 0 && l <= h) {
      atomicMin(bounds + j, ordered_bits(l));
      atomicMax(bounds + 3 + j, ordered_bits(h));
    }
  }
}

// ---- one crop round: x = scaled - min (the reference's `xyz -= xyz.min(0)`), then
// form 1: all_j(x + off >= 0) and all_j(x + off < full_scale);  form 2: lo <= x <= hi on columns 0 and 1
__global__ __launch_bounds__(SP_BLOCK) void sp_crop_mask_kernel(const double* __restrict__ scaled, int64_t n, D3 mn,
                                                                int form, D3 a, D3 b, uint8_t* __restrict__ mask,
                                                                unsigned long long* __restrict__ round) {
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double kmin[3] = {inf, inf, inf};
  int cnt = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double x[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = scaled[3 * i + j] - mn.v[j];
    bool ok = true;
    if (form == 1) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double t = x[j] + a.v[j];
        ok = ok && t >= 0.0 && t < b.v[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) ok = ok && x[j] >= a.v[j] && x[j] <= b.v[j];
    }
    mask[i] = ok ? 1 : 0;
    if (ok) {
      ++cnt;
#pragma unroll
      for (int j = 0; j < 3; ++j) kmin[j] = x[j] < kmin[j] ? x[j] : kmin[j];
    }
  }
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
#pragma unroll
  for (int j = 0; j < 3; ++j) kmin[j] = wave_min(kmin[j]);
  if (lane == 0 && cnt) {
    atomicAdd(round, (unsigned long long)cnt);
#pragma unroll
    for (int j = 0; j < 3; ++j) atomicMin(round + 1 + j, ordered_bits(kmin[j]));
  }
}

// ---- order-preserving compaction.  A workgroup owns SP_TILE consecutive points, a thread SP_PER consecutive ones.
__device__ __forceinline__ int sp_kept(const uint8_t* __restrict__ mask, int64_t i, int64_t n) {
  return i < n ? (mask ? (mask[i] != 0) : 1) : 0;
}

__global__ __launch_bounds__(SP_BLOCK) void sp_tile_count_kernel(const uint8_t* __restrict__ mask, int64_t n,
                                                                 int32_t* __restrict__ tile_count) {
  __shared__ int s_w[SP_WAVES];
  const int64_t base = (int64_t)blockIdx.x * SP_TILE + (int64_t)threadIdx.x * SP_PER;
  int c = 0;
#pragma unroll
  for (int k = 0; k < SP_PER; ++k) c += sp_kept(mask, base + k, n);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < SP_WAVES; ++w) t += s_w[w];
    tile_count[blockIdx.x] = t;
  }
}

struct EmitArgs {
  const uint8_t* mask;
  const int32_t* tile_count;
  const int64_t* pick;
  const double* scaled;
  const double* middle;
  const float* rgb;
  const int64_t* sem;
  const int64_t* ins;
  const int64_t* sp;
  int64_t n, n_src, n_out, S, n_ids;
  D3 mn, off;
  F3 jit;
  int64_t* loc;
  float* loc_float;
  double* middle_kept;
  float* feat;
  int64_t* sem_out;
  int64_t* ins_raw;
  int64_t* sp_old;
  int32_t* sp_flag;
  int32_t* ins_flag;
  unsigned long long* st;
};

__global__ __launch_bounds__(SP_BLOCK) void sp_emit_kernel(EmitArgs A) {
  __shared__ long long s_red[SP_WAVES];
  __shared__ int s_w[SP_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // first output row of this tile: the kept points of all earlier tiles (a few hundred tiles per scene)
  long long before = 0;
  if (A.mask) {
    for (int64_t t = tid; t < (int64_t)blockIdx.x; t += SP_BLOCK) before += A.tile_count[t];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) before += __shfl_xor(before, m);
    if (lane == 0) s_red[wave] = before;
    __syncthreads();
    before = 0;
#pragma unroll
    for (int w = 0; w < SP_WAVES; ++w) before += s_red[w];
  } else {
    before = (long long)blockIdx.x * SP_TILE;
  }
  const int64_t base = (int64_t)blockIdx.x * SP_TILE + (int64_t)tid * SP_PER;
  int keep[SP_PER], c = 0;
#pragma unroll
  for (int k = 0; k < SP_PER; ++k) {
    keep[k] = sp_kept(A.mask, base + k, A.n);
    c += keep[k];
  }
  // exclusive scan of c over the workgroup: inclusive wave scan, then the totals of the earlier waves
  int inc = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int excl = inc - c;
  for (int w = 0; w < wave; ++w) excl += s_w[w];
  int64_t o = before + excl;
  long long lmax[3] = {0, 0, 0};
  int bad = 0;
#pragma unroll
  for (int k = 0; k < SP_PER; ++k) {
    if (!keep[k]) continue;
    const int64_t i = base + k;
    if (o >= A.n_out) {                      // more ones in the mask than the caller made room for
      bad = 1;
      continue;
    }
    int64_t p = A.pick ? A.pick[i] : i;
    if (p < 0 || p >= A.n_src) {
      p = 0;
      bad = 1;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double x = (A.scaled[3 * i + j] - A.mn.v[j]) + A.off.v[j];
      const long long v = (long long)x;      // toward zero, as torch's .long()
      A.loc[3 * o + j] = v;
      lmax[j] = v > lmax[j] ? v : lmax[j];
      const double mid = A.middle[3 * i + j];
      A.middle_kept[3 * o + j] = mid;
      A.loc_float[3 * o + j] = (float)mid;
      const float f = A.rgb[3 * p + j];
      A.feat[3 * o + j] = A.jit.on ? f + A.jit.v[j] : f;
    }
    A.sem_out[o] = A.sem[p];
    const int64_t id = A.ins[p], s = A.sp[p];
    A.ins_raw[o] = id;
    A.sp_old[o] = s;
    if (s >= 0 && s < A.S) A.sp_flag[s] = 1; else bad = 1;
    if (id >= 0) {
      if (id < A.n_ids) A.ins_flag[id] = 1; else bad = 1;
    }
    ++o;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const long long t = __shfl_xor(lmax[j], m);
      lmax[j] = t > lmax[j] ? t : lmax[j];
    }
    if (lane == 0 && lmax[j] > 0) atomicMax(A.st + ST_LOCMAX + j, (unsigned long long)lmax[j]);
  }
  const unsigned long long b = __ballot(bad);
  if (lane == 0 && b) atomicAdd(A.st + ST_BAD, (unsigned long long)__popcll(b));
}

// ---- the two id tables, one workgroup.  Exclusive scan of 0/1 flags in global memory, SP_SCAN_BLOCK at a time.
__device__ int sp_block_scan_flags(const int32_t* __restrict__ flag, int64_t n, int32_t* __restrict__ rank, int* s_w,
                                   int* s_carry) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) *s_carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < n; base += SP_SCAN_BLOCK) {
    const int64_t i = base + tid;
    const int f = (i < n && flag[i] != 0) ? 1 : 0;
    const unsigned long long bal = __ballot(f);
    const int inw = __popcll(bal & ((1ull << lane) - 1ull));      // kept lanes below this one
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int excl = *s_carry + inw;
    for (int w = 0; w < wave; ++w) excl += s_w[w];
    if (i < n) rank[i] = excl;
    __syncthreads();
    if (tid == SP_SCAN_BLOCK - 1) *s_carry = excl + f;
    __syncthreads();
  }
  return *s_carry;
}

__global__ __launch_bounds__(SP_SCAN_BLOCK) void sp_tables_kernel(const int32_t* __restrict__ sp_flag, int64_t S,
                                                                  const int32_t* __restrict__ ins_flag, int64_t n_ids,
                                                                  int32_t* __restrict__ sp_new,
                                                                  int64_t* __restrict__ subset,
                                                                  int32_t* __restrict__ ins_rank,
                                                                  int32_t* __restrict__ hole,
                                                                  int32_t* __restrict__ ins_map,
                                                                  unsigned long long* __restrict__ st) {
  __shared__ int s_w[SP_SCAN_BLOCK / 64];
  __shared__ int s_carry;
  const int tid = threadIdx.x;
  // np.unique(superpoint, return_inverse=True): ascending kept ids, their ranks
  const int s_new = sp_block_scan_flags(sp_flag, S, sp_new, s_w, &s_carry);
  __syncthreads();
  for (int64_t i = tid; i < S; i += SP_SCAN_BLOCK) {
    if (sp_flag[i] != 0) subset[sp_new[i]] = i; else sp_new[i] = -1;
  }
  // get_cropped_inst_label: with k ids present the result uses 0..k-1.  Walking j upward, the i-th empty id below k
  // takes the i-th LARGEST present id, and those are exactly the present ids >= k; ids below k keep their value.
  const int k = sp_block_scan_flags(ins_flag, n_ids, ins_rank, s_w, &s_carry);
  __syncthreads();
  for (int64_t j = tid; j < n_ids; j += SP_SCAN_BLOCK)
    if (ins_flag[j] == 0 && j < k) hole[j - ins_rank[j]] = (int32_t)j;
  __syncthreads();
  for (int64_t j = tid; j < n_ids; j += SP_SCAN_BLOCK) {
    int32_t v = -1;
    if (ins_flag[j] != 0) v = j < k ? (int32_t)j : hole[k - 1 - ins_rank[j]];
    ins_map[j] = v;
  }
  if (tid == 0) {
    st[ST_SNEW] = (unsigned long long)s_new;
    st[ST_KINST] = (unsigned long long)k;
  }
}

__global__ void sp_relabel_kernel(const int64_t* __restrict__ sp_old, const int64_t* __restrict__ ins_raw, int64_t n,
                                  const int32_t* __restrict__ sp_new, int64_t S, const int32_t* __restrict__ ins_map,
                                  int64_t n_ids, int64_t* __restrict__ sp_out, int64_t* __restrict__ ins_out,
                                  int64_t* __restrict__ seg) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = sp_old[i], id = ins_raw[i];
    sp_out[i] = (s >= 0 && s < S) ? sp_new[s] : -1;
    int64_t v = id;                                                // -100 (any negative label) passes through
    if (id >= 0) v = id < n_ids ? ins_map[id] : -1;
    ins_out[i] = v;
    seg[i] = (v >= 0 && v < n_ids) ? v : n_ids;                    // the row of the points without an instance
  }
}

// ---- get_instance_info: one wave per instance id (row K: the points without an instance)
__global__ __launch_bounds__(SP_BLOCK) void sp_instance_info_kernel(const double* __restrict__ mid,
                                                                    const int32_t* __restrict__ perm,
                                                                    const int32_t* __restrict__ offsets, int64_t K,
                                                                    float* __restrict__ info,
                                                                    int32_t* __restrict__ pointnum) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
  if (r > K) return;
  const int b = offsets[r], e = offsets[r + 1];
  float out[9];
  if (r == K) {
#pragma unroll
    for (int c = 0; c < 9; ++c) out[c] = -100.0f;
  } else {
    if (lane == 0) pointnum[r] = e - b;
    if (e == b) return;                                            // an id without points: no row to write
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double s[3] = {0.0, 0.0, 0.0}, lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int j = b + lane; j < e; j += 64) {
      const int64_t p = perm[j];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v = mid[3 * p + c];
        s[c] += v;
        lo[c] = v < lo[c] ? v : lo[c];
        hi[c] = v > hi[c] ? v : hi[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) s[c] += __shfl_xor(s[c], m);
      out[c] = (float)(s[c] / (double)(e - b));
      out[3 + c] = (float)wave_min(lo[c]);
      out[6 + c] = (float)wave_max(hi[c]);
    }
  }
  for (int j = b + lane; j < e; j += 64) {
    const int64_t p = perm[j];
#pragma unroll
    for (int c = 0; c < 9; ++c) info[9 * p + c] = out[c];
  }
}

inline D3 d3(const double* h) {
  D3 r;
  for (int j = 0; j < 3; ++j) r.v[j] = h ? h[j] : 0.0;
  return r;
}

// cells of one elastic grid: bb >= 3 per axis and fewer than 2^31 cells per grid; 0 where the shape is refused
inline int64_t elastic_cells(const int32_t* bb) {
  int64_t c = 1;
  for (int j = 0; j < 3; ++j) {
    if (bb[j] < 3) return 0;
    c *= bb[j];
    if (c >= ((int64_t)1 << 31)) return 0;
  }
  return c;
}

}  // namespace

extern "C" {

int64_t wsis_sp_state_bytes(void) { return (int64_t)WSIS_SP_STATE_WORDS * 8; }

int wsis_sp_state_init(void* d_state, void* stream) {
  WSIS_REQUIRE(d_state, "null pointer");
  static_assert(WSIS_SP_STATE_WORDS <= SP_BLOCK && WSIS_SP_STATE_WORDS == ST_ROUND0 + 4 * WSIS_SP_ROUNDS, "state layout");
  hipLaunchKernelGGL(sp_state_init_kernel, dim3(1), dim3(SP_BLOCK), 0, as_stream(stream),
                     static_cast<unsigned long long*>(d_state));
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_sp_affine(const void* d_in, int32_t in_f64, const int64_t* d_pick, int64_t n_src, int64_t n, const double* h_m9,
                   double scale, double* d_middle, double* d_scaled, void* d_state, void* stream) {
  WSIS_REQUIRE(n >= 0 && n_src >= 0, "negative size");
  WSIS_REQUIRE(n < ((int64_t)1 << 31) && n_src < ((int64_t)1 << 31), "sizes exceed int32");
  WSIS_REQUIRE(d_pick || n <= n_src, "n > n_src without an index vector");
  WSIS_REQUIRE(h_m9, "null matrix");
  WSIS_REQUIRE(!d_scaled || d_state, "bounds need the state block");
  if (n == 0) return WSIS_OK;
  WSIS_REQUIRE(n_src > 0 && d_in && d_middle, "null pointer");
  M9 a;
  for (int j = 0; j < 9; ++j) a.m[j] = h_m9[j];
  unsigned long long* st = static_cast<unsigned long long*>(d_state);
  const dim3 g(grid_for(n, SP_BLOCK)), b(SP_BLOCK);
  if (in_f64)
    hipLaunchKernelGGL(sp_affine_kernel<double>, g, b, 0, as_stream(stream), static_cast<const double*>(d_in), d_pick,
                       n_src, n, a, scale, d_middle, d_scaled, st);
  else
    hipLaunchKernelGGL(sp_affine_kernel<float>, g, b, 0, as_stream(stream), static_cast<const float*>(d_in), d_pick,
                       n_src, n, a, scale, d_middle, d_scaled, st);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_elastic_blur(float* d_grids, float* d_tmp, const int32_t* h_bb3, void* stream) {
  WSIS_REQUIRE(d_grids && d_tmp && h_bb3, "null pointer");
  WSIS_REQUIRE(d_grids != d_tmp, "the workspace is the grids");
  const int64_t cells = elastic_cells(h_bb3);
  WSIS_REQUIRE(cells > 0, "a grid side below 3, or 2^31 cells or more");
  const dim3 g((unsigned)ceil_div(cells, EL_BLOCK), 3), b(EL_BLOCK);
  float *src = d_grids, *dst = d_tmp;
  for (int pass = 0; pass < 6; ++pass) {                            // axis 0, 1, 2, 0, 1, 2: the result is in d_grids again
    const int axis = pass % 3;
    const int64_t stride = axis == 0 ? (int64_t)h_bb3[1] * h_bb3[2] : (axis == 1 ? (int64_t)h_bb3[2] : 1);
    hipLaunchKernelGGL(sp_elastic_blur_kernel, g, b, 0, as_stream(stream), src, dst, cells, stride, (int)h_bb3[axis]);
    WSIS_LAUNCH_CHECK();
    float* t = src;
    src = dst;
    dst = t;
  }
  return WSIS_OK;
}

int wsis_elastic_apply(double* d_xyz, int64_t n, const float* d_grids, const int32_t* h_bb3, int32_t gran, double mag,
                          void* d_bounds, void* stream) {
  WSIS_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad n");
  WSIS_REQUIRE(h_bb3 && d_bounds, "null pointer");
  WSIS_REQUIRE(elastic_cells(h_bb3) > 0, "a grid side below 3, or 2^31 cells or more");
  WSIS_REQUIRE(gran >= 1, "gran < 1");
  for (int j = 0; j < 3; ++j)                                      // the nodes are integers fp64 holds exactly
    WSIS_REQUIRE(((int64_t)h_bb3[j] - 1) * (int64_t)gran < ((int64_t)1 << 52), "grid extent exceeds 2^52");
  unsigned long long* bounds = static_cast<unsigned long long*>(d_bounds);
  WSIS_HIP_CHECK(hipMemsetAsync(bounds, 0xff, 3 * sizeof(unsigned long long), as_stream(stream)));   // minima: largest key
  WSIS_HIP_CHECK(hipMemsetAsync(bounds + 3, 0, 3 * sizeof(unsigned long long), as_stream(stream)));
  if (n == 0) return WSIS_OK;
  WSIS_REQUIRE(d_xyz && d_grids, "null pointer");
  I3 bb;
  D3 first;
  for (int j = 0; j < 3; ++j) {
    bb.v[j] = h_bb3[j];
    first.v[j] = (double)(-((int64_t)h_bb3[j] - 1) * (int64_t)gran);
  }
  hipLaunchKernelGGL(sp_elastic_apply_kernel, dim3((unsigned)ceil_div(n, EL_BLOCK)), dim3(EL_BLOCK), 0,
                     as_stream(stream), d_xyz, n, d_grids, bb, first, 2.0 * (double)gran, mag, bounds);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_sp_crop_mask(const double* d_scaled, int64_t n, const double* h_min3, int32_t form, const double* h_a3,
                      const double* h_b3, uint8_t* d_mask, void* d_state, int32_t round, void* stream) {
  WSIS_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "bad n");
  WSIS_REQUIRE(form == 1 || form == 2, "form is 1 (crop) or 2 (crop_v2)");
  WSIS_REQUIRE(round >= 0 && round < WSIS_SP_ROUNDS, "round outside the state block");
  WSIS_REQUIRE(h_min3 && h_a3 && h_b3 && d_state, "null pointer");
  if (n == 0) return WSIS_OK;
  WSIS_REQUIRE(d_scaled && d_mask, "null pointer");
  hipLaunchKernelGGL(sp_crop_mask_kernel, dim3(grid_for(n, SP_BLOCK)), dim3(SP_BLOCK), 0, as_stream(stream), d_scaled, n,
                     d3(h_min3), (int)form, d3(h_a3), d3(h_b3), d_mask,
                     static_cast<unsigned long long*>(d_state) + ST_ROUND0 + 4 * round);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_sp_emit_workspace_bytes(int64_t n, int64_t S, int64_t n_ids) {
  if (n < 0 || S < 0 || n_ids < 0 || n_ids > WSIS_SP_MAX_IDS || n >= ((int64_t)1 << 31) || S >= ((int64_t)1 << 31))
    return -1;
  return (int64_t)sizeof(int32_t) * (ceil_div(n, SP_TILE) + 1);
}

int wsis_sp_emit(const uint8_t* d_mask, const int64_t* d_pick, int64_t n_src, int64_t n, int64_t n_out,
                 const double* d_scaled, const double* d_middle, const double* h_min3, const double* h_off3,
                 const float* d_rgb, const float* h_jitter3, const int64_t* d_sem, const int64_t* d_ins,
                 const int64_t* d_sp, int64_t S, int64_t n_ids, int64_t* d_loc, float* d_loc_float,
                 double* d_middle_kept, float* d_feat, int64_t* d_sem_out, int64_t* d_ins_raw, int64_t* d_sp_old,
                 int32_t* d_flags, void* d_state, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(n >= 0 && n_src >= 0 && n_out >= 0 && S >= 0 && n_ids >= 0, "negative size");
  WSIS_REQUIRE(n < ((int64_t)1 << 31) && n_src < ((int64_t)1 << 31) && S < ((int64_t)1 << 31), "sizes exceed int32");
  if (n_ids > WSIS_SP_MAX_IDS) return ::wsis::fail(WSIS_ERR_OVERFLOW, "wsis_sp_emit: more than 65536 instance ids");
  WSIS_REQUIRE(d_pick || n <= n_src, "n > n_src without an index vector");
  WSIS_REQUIRE(d_mask || n_out >= n, "no room for every point");
  WSIS_REQUIRE(d_state && h_min3 && h_off3 && (S + n_ids == 0 || d_flags), "null pointer");
  hipStream_t st = as_stream(stream);
  if (S + n_ids > 0) WSIS_HIP_CHECK(hipMemsetAsync(d_flags, 0, (size_t)(S + n_ids) * sizeof(int32_t), st));
  if (n == 0) return WSIS_OK;
  WSIS_REQUIRE(d_scaled && d_middle && d_rgb && d_sem && d_ins && d_sp, "null input");
  WSIS_REQUIRE(n_out == 0 || (d_loc && d_loc_float && d_middle_kept && d_feat && d_sem_out && d_ins_raw && d_sp_old),
               "null output");
  const int64_t tiles = ceil_div(n, SP_TILE);
  int32_t* tile_count = static_cast<int32_t*>(d_ws);
  if (d_mask) {
    WSIS_REQUIRE(d_ws && ws_bytes >= wsis_sp_emit_workspace_bytes(n, S, n_ids), "workspace too small");
    hipLaunchKernelGGL(sp_tile_count_kernel, dim3((unsigned)tiles), dim3(SP_BLOCK), 0, st, d_mask, n, tile_count);
    WSIS_LAUNCH_CHECK();
  }
  EmitArgs A;
  A.mask = d_mask;
  A.tile_count = tile_count;
  A.pick = d_pick;
  A.scaled = d_scaled;
  A.middle = d_middle;
  A.rgb = d_rgb;
  A.sem = d_sem;
  A.ins = d_ins;
  A.sp = d_sp;
  A.n = n;
  A.n_src = n_src;
  A.n_out = n_out;
  A.S = S;
  A.n_ids = n_ids;
  A.mn = d3(h_min3);
  A.off = d3(h_off3);
  A.jit.on = h_jitter3 ? 1 : 0;
  for (int j = 0; j < 3; ++j) A.jit.v[j] = h_jitter3 ? h_jitter3[j] : 0.f;
  A.loc = d_loc;
  A.loc_float = d_loc_float;
  A.middle_kept = d_middle_kept;
  A.feat = d_feat;
  A.sem_out = d_sem_out;
  A.ins_raw = d_ins_raw;
  A.sp_old = d_sp_old;
  A.sp_flag = d_flags;
  A.ins_flag = d_flags + S;
  A.st = static_cast<unsigned long long*>(d_state);
  hipLaunchKernelGGL(sp_emit_kernel, dim3((unsigned)tiles), dim3(SP_BLOCK), 0, st, A);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_sp_tables(const int32_t* d_flags, int64_t S, int64_t n_ids, int32_t* d_sp_new, int64_t* d_subset,
                   int32_t* d_ins_map, int32_t* d_scratch, void* d_state, void* stream) {
  WSIS_REQUIRE(S >= 0 && n_ids >= 0 && S < ((int64_t)1 << 31), "bad size");
  if (n_ids > WSIS_SP_MAX_IDS) return ::wsis::fail(WSIS_ERR_OVERFLOW, "wsis_sp_tables: more than 65536 instance ids");
  WSIS_REQUIRE(d_state, "null pointer");
  WSIS_REQUIRE(S + n_ids == 0 || d_flags, "null pointer");
  WSIS_REQUIRE(S == 0 || (d_sp_new && d_subset), "null pointer");
  WSIS_REQUIRE(n_ids == 0 || (d_ins_map && d_scratch), "null pointer");
  hipLaunchKernelGGL(sp_tables_kernel, dim3(1), dim3(SP_SCAN_BLOCK), 0, as_stream(stream), d_flags, S, d_flags + S,
                     n_ids, d_sp_new, d_subset, d_scratch, d_scratch + n_ids, d_ins_map,
                     static_cast<unsigned long long*>(d_state));
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_sp_relabel(const int64_t* d_sp_old, const int64_t* d_ins_raw, int64_t n, const int32_t* d_sp_new, int64_t S,
                    const int32_t* d_ins_map, int64_t n_ids, int64_t* d_sp_out, int64_t* d_ins_out, int64_t* d_seg,
                    void* stream) {
  WSIS_REQUIRE(n >= 0 && S >= 0 && n_ids >= 0 && n_ids <= WSIS_SP_MAX_IDS, "bad size");
  if (n == 0) return WSIS_OK;
  WSIS_REQUIRE(d_sp_old && d_ins_raw && d_sp_out && d_ins_out && d_seg && (S == 0 || d_sp_new) && (n_ids == 0 || d_ins_map),
               "null pointer");
  hipLaunchKernelGGL(sp_relabel_kernel, dim3(grid_for(n, SP_BLOCK)), dim3(SP_BLOCK), 0, as_stream(stream), d_sp_old,
                     d_ins_raw, n, d_sp_new, S, d_ins_map, n_ids, d_sp_out, d_ins_out, d_seg);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_sp_instance_info(const double* d_middle, const int32_t* d_perm, const int32_t* d_offsets, int64_t n, int64_t K,
                          float* d_info, int32_t* d_pointnum, void* stream) {
  WSIS_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && K >= 0 && K <= WSIS_SP_MAX_IDS, "bad size");
  if (n == 0) {
    if (K > 0) {
      WSIS_REQUIRE(d_pointnum, "null pointer");
      WSIS_HIP_CHECK(hipMemsetAsync(d_pointnum, 0, (size_t)K * sizeof(int32_t), as_stream(stream)));
    }
    return WSIS_OK;
  }
  WSIS_REQUIRE(d_middle && d_perm && d_offsets && d_info && (K == 0 || d_pointnum), "null pointer");
  hipLaunchKernelGGL(sp_instance_info_kernel, dim3((unsigned)ceil_div(K + 1, SP_WAVES)), dim3(SP_BLOCK), 0,
                     as_stream(stream), d_middle, d_perm, d_offsets, K, d_info, d_pointnum);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
