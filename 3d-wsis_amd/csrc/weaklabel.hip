// The three weak-label stage updates of the training schedule (modules/datasets/scannetv2_dataset.py of the reference,
// called from train_scannetv2.py:477-480, 575-577, 664-666; the S3DIS dataset has the same methods):
//
//   extend_label_to_neighbor / propagate_label_to_neighbor  :780-865   wsis_wl_neighbor_source + wsis_wl_apply_source
//   the graph-writing tail of weak_label_propagation         :739-772   wsis_wl_apply_source
//   propagate_label_to_whole_scene                           :873-964   wsis_wl_scene_assign
//   generate_point_level_weak_label                          :568-595   wsis_wl_point_labels
//   cal_occupancy / cal_instance_size                        :515-564   wsis_wl_occupancy / wsis_wl_instance_size
//   the label statistics                                     :602-640   wsis_wl_label_stats
//
// The reference forms one boolean mask `superpoint == spID` per superpoint and use: O(S*N) per scene.  Here every
// per-point stage is ONE pass over the points (through the superpoint CSR for the coordinate sums), and everything else
// is O(S + E) or O(S*P) work on per-superpoint arrays (P = number of labelled superpoints, the "priors").
//
// Reproducibility: no floating-point atomic anywhere.  The per-superpoint sums are one wave per superpoint with a
// fixed lane assignment and one fixed-order butterfly; the pseudo instance centres are added by one wave per prior in
// ascending superpoint order; integer atomics are used only where the result does not depend on their order (max of a
// superpoint id, max of the bit pattern of a non-negative double, counters).  Distances are evaluated in fp64 as
// sqrt((dx*dx + dy*dy) + dz*dz), uncontracted (-ffp-contract=off), which is numpy's norm of a 3-vector bit for bit.
#include "common.h"

using namespace wsis;

namespace {

constexpr int WL_BLOCK = 256;
constexpr int WL_WAVES = WL_BLOCK / 64;
constexpr int WL_SEARCH_BLOCK = 64;              // one wave per workgroup, one superpoint per lane: S is a few thousand
constexpr int WL_PC = 256;                       // priors staged in LDS at a time (8 KiB)
constexpr int WL_NSTAT = 8;
constexpr int WL_STUFF_MAX = 8;
constexpr int64_t WL_NONE = -100;

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ __forceinline__ bool wl_labelled(int64_t sem, int64_t ins) { return sem != WL_NONE && ins != WL_NONE; }

// ---- per-superpoint coordinate sum / count / centre: one wave per superpoint, lane l takes the points l, l + 64, ...
// of the CSR row in order, then one xor butterfly (both partners add the same pair: every lane ends with the same value)
__global__ __launch_bounds__(WL_BLOCK) void wl_sp_stats_kernel(const float* __restrict__ xyz,
                                                               const int32_t* __restrict__ perm,
                                                               const int32_t* __restrict__ offsets, int64_t S,
                                                               float* __restrict__ sum, int32_t* __restrict__ count,
                                                               float* __restrict__ centre) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * WL_WAVES + (threadIdx.x >> 6);
  if (s >= S) return;
  const int b = offsets[s], e = offsets[s + 1];
  float x = 0.f, y = 0.f, z = 0.f;
  for (int j = b + lane; j < e; j += 64) {
    const int64_t p = perm[j];
    x += xyz[3 * p];
    y += xyz[3 * p + 1];
    z += xyz[3 * p + 2];
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float tx = __shfl_xor(x, m), ty = __shfl_xor(y, m), tz = __shfl_xor(z, m);
    x += tx;
    y += ty;
    z += tz;
  }
  if (lane == 0) {
    const float n = (float)(e - b);              // an empty superpoint gives NaN, as the reference's mean does
    sum[3 * s] = x;
    sum[3 * s + 1] = y;
    sum[3 * s + 2] = z;
    count[s] = e - b;
    centre[3 * s] = x / n;
    centre[3 * s + 1] = y / n;
    centre[3 * s + 2] = z / n;
  }
}

// ---- neighbour stage: src[n] = the largest labelled k adjacent to the unlabelled n (either edge direction) with
// sem[k] == pred[n] (and conf[n] > thr).  The reference visits k ascending and the last writer wins: a max.
__device__ __forceinline__ void wl_offer(int64_t k, int64_t n, const int64_t* __restrict__ sem,
                                         const int64_t* __restrict__ ins, const int64_t* __restrict__ pred,
                                         const float* __restrict__ conf, double thr, int32_t* __restrict__ src) {
  if (!wl_labelled(sem[k], ins[k])) return;
  if (sem[n] != WL_NONE || ins[n] != WL_NONE) return;
  if (sem[k] != pred[n]) return;
  if (conf && !((double)conf[n] > thr)) return;
  atomicMax(src + n, (int32_t)k);
}

__global__ void wl_neighbor_kernel(const int64_t* __restrict__ edges, int64_t E, const int64_t* __restrict__ sem,
                                   const int64_t* __restrict__ ins, const int64_t* __restrict__ pred,
                                   const float* __restrict__ conf, double thr, int64_t S, int32_t* __restrict__ src) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = edges[2 * e], b = edges[2 * e + 1];
    if (a < 0 || a >= S || b < 0 || b >= S) continue;
    wl_offer(a, b, sem, ins, pred, conf, thr, src);
    wl_offer(b, a, sem, ins, pred, conf, thr, src);
  }
}

__global__ void wl_apply_kernel(const int32_t* __restrict__ src, const int64_t* __restrict__ sem,
                                const int64_t* __restrict__ ins, const double* __restrict__ off,
                                const float* __restrict__ centre, int64_t S, int64_t* __restrict__ sem_out,
                                int64_t* __restrict__ ins_out, double* __restrict__ off_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < S; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = src[i];
    const bool take = k >= 0 && k < S;
    const int64_t from = take ? k : i;
    sem_out[i] = sem[from];
    ins_out[i] = ins[from];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      off_out[3 * i + j] = take ? ((double)centre[3 * k + j] + off[3 * k + j]) - (double)centre[3 * i + j] : off[3 * i + j];
  }
}

__global__ void wl_is1ins_kernel(const int64_t* __restrict__ edges, int64_t E, const int64_t* __restrict__ ins, int64_t S,
                                 int64_t* __restrict__ is1ins) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = edges[2 * e], b = edges[2 * e + 1];
    int64_t v = 0;
    if (a >= 0 && a < S && b >= 0 && b < S) {
      const int64_t ia = ins[a], ib = ins[b];
      v = (ia == WL_NONE || ib == WL_NONE) ? 0 : (ia == ib ? -1 : 1);
    }
    is1ins[e] = v;
  }
}

// ---- whole-scene stage, search: one superpoint per lane; the workgroup stages WL_PC priors at a time in LDS as
// (fp64 instance centre, class) and every lane walks the chunk -- all lanes read the same LDS address (a broadcast, no
// bank conflict).  `d < best` is strict and the priors are walked in index order: the first of equal distances wins.
__global__ __launch_bounds__(WL_SEARCH_BLOCK) void wl_scene_search_kernel(
    const int32_t* __restrict__ prior, int P, const int64_t* __restrict__ sem, const int64_t* __restrict__ ins,
    const double* __restrict__ off, const float* __restrict__ centre, const int64_t* __restrict__ pred,
    const float* __restrict__ pred_off, double max_dist, int64_t S, int32_t* __restrict__ assigned,
    double* __restrict__ dist, int64_t* __restrict__ sem_out, int64_t* __restrict__ ins_out, double* __restrict__ off_out) {
  __shared__ double s_c[WL_PC * 3];
  __shared__ int64_t s_sem[WL_PC];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * WL_SEARCH_BLOCK + tid;
  const bool active = i < S;
  bool open = false;
  double qx = 0.0, qy = 0.0, qz = 0.0;
  int64_t want = WL_NONE;
  if (active) {
    sem_out[i] = sem[i];
    ins_out[i] = ins[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) off_out[3 * i + j] = off[3 * i + j];
    open = !wl_labelled(sem[i], ins[i]);
    qx = (double)(centre[3 * i] + pred_off[3 * i]);              // the reference's sum is an fp32 one
    qy = (double)(centre[3 * i + 1] + pred_off[3 * i + 1]);
    qz = (double)(centre[3 * i + 2] + pred_off[3 * i + 2]);
    want = pred[i];
  }
  double best = __longlong_as_double(0x7ff0000000000000ll);      // +inf: no candidate
  int bi = -1;
  for (int p0 = 0; p0 < P; p0 += WL_PC) {
    const int pc = min(WL_PC, P - p0);
    __syncthreads();                                             // the previous chunk has been read
    for (int t = tid; t < pc; t += WL_SEARCH_BLOCK) {
      const int64_t k = prior[p0 + t];
#pragma unroll
      for (int j = 0; j < 3; ++j) s_c[3 * t + j] = (double)centre[3 * k + j] + off[3 * k + j];
      s_sem[t] = sem[k];
    }
    __syncthreads();
    if (open) {
      for (int t = 0; t < pc; ++t) {
        if (s_sem[t] != want) continue;
        const double dx = s_c[3 * t] - qx, dy = s_c[3 * t + 1] - qy, dz = s_c[3 * t + 2] - qz;
        const double d = sqrt((dx * dx + dy * dy) + dz * dz);
        if (d < best) {
          best = d;
          bi = p0 + t;
        }
      }
    }
  }
  if (active) {
    assigned[i] = (bi >= 0 && !(best > max_dist)) ? bi : -1;
    dist[i] = best;
  }
}

// ---- whole-scene stage, pseudo instance centres: one wave per prior.  Pass 1 walks the superpoints 64 at a time, a
// ballot marks the ones assigned to this prior and their fp32 sums are added in ascending id order (every lane does the
// same additions); pass 2 walks them again and each assigned superpoint writes its own row.
__global__ __launch_bounds__(WL_BLOCK) void wl_scene_gather_kernel(
    const int32_t* __restrict__ prior, int P, const int32_t* __restrict__ assigned, const float* __restrict__ sum,
    const int32_t* __restrict__ count, const float* __restrict__ centre, const int64_t* __restrict__ sem,
    const int64_t* __restrict__ ins, int64_t S, int64_t* __restrict__ sem_out, int64_t* __restrict__ ins_out,
    double* __restrict__ off_out) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * WL_WAVES + (threadIdx.x >> 6);
  if (p >= P) return;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  int64_t n = 0;
  for (int64_t base = 0; base < S; base += 64) {
    const int64_t i = base + lane;
    unsigned long long mask = __ballot(i < S && assigned[i] == p);
    while (mask) {
      const int64_t ii = base + (__ffsll(mask) - 1);
      mask &= mask - 1;
      gx += (double)sum[3 * ii];
      gy += (double)sum[3 * ii + 1];
      gz += (double)sum[3 * ii + 2];
      n += count[ii];
    }
  }
  if (n == 0) return;                                            // wave-uniform
  gx /= (double)n;
  gy /= (double)n;
  gz /= (double)n;
  const int64_t k = prior[p];
  const int64_t sk = sem[k], ik = ins[k];
  for (int64_t base = 0; base < S; base += 64) {
    const int64_t i = base + lane;
    if (i < S && assigned[i] == p) {
      sem_out[i] = sk;
      ins_out[i] = ik;
      off_out[3 * i] = gx - (double)centre[3 * i];
      off_out[3 * i + 1] = gy - (double)centre[3 * i + 1];
      off_out[3 * i + 2] = gz - (double)centre[3 * i + 2];
    }
  }
}

// ---- point-level weak labels: one gather per point
__global__ void wl_point_labels_kernel(const int64_t* __restrict__ sp, int64_t N, const int64_t* __restrict__ sem,
                                       const int64_t* __restrict__ ins, double* __restrict__ weak_sem,
                                       double* __restrict__ weak_ins) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = sp[i];
    const bool lab = wl_labelled(sem[s], ins[s]);
    weak_sem[i] = lab ? (double)sem[s] : -100.0;
    weak_ins[i] = lab ? (double)ins[s] : -100.0;
  }
}

// ---- occupancy keys: (rank of the point's weak instance label, trunc(float32(xyz) * float32(scale))): the conversion
// to integer truncates toward zero, as torch's .long() of the reference does
__global__ void wl_keys_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ sp,
                               const int32_t* __restrict__ rank_sp, int64_t N, float scale, int64_t* __restrict__ coords) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    coords[4 * i] = rank_sp[sp[i]];
    coords[4 * i + 1] = (int64_t)(xyz[3 * i] * scale);
    coords[4 * i + 2] = (int64_t)(xyz[3 * i + 1] * scale);
    coords[4 * i + 3] = (int64_t)(xyz[3 * i + 2] * scale);
  }
}

// the first point to reach a voxel counts it for the voxel's label rank (integer atomics: the counts are exact)
__global__ void wl_voxel_count_kernel(const int32_t* __restrict__ p2v, const int64_t* __restrict__ coords, int64_t N,
                                      int32_t R, int32_t* __restrict__ seen, unsigned long long* __restrict__ vox_count) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = coords[4 * i];
    if (r < 0 || r >= R) continue;
    if (atomicExch(seen + p2v[i], 1) == 0) atomicAdd(vox_count + r, 1ull);
  }
}

// ---- instance size: max of ||off_v|| over the vertices of a label.  The norms are non-negative doubles, whose order is
// the order of their bit patterns as unsigned integers: an integer atomicMax, whatever the order of arrival
__global__ void wl_size_max_kernel(const double* __restrict__ off, const int32_t* __restrict__ rank, int64_t S, int32_t R,
                                   unsigned long long* __restrict__ rmax_bits) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < S; v += (int64_t)gridDim.x * blockDim.x) {
    const int32_t r = rank[v];
    if (r < 0 || r >= R) continue;
    const double x = off[3 * v], y = off[3 * v + 1], z = off[3 * v + 2];
    const double n = sqrt((x * x + y * y) + z * z);
    if (n > 0.0) atomicMax(rmax_bits + r, (unsigned long long)__double_as_longlong(n));
  }
}

__global__ void wl_size_gather_kernel(const double* __restrict__ rmax, const int32_t* __restrict__ rank, int64_t S,
                                      int32_t R, double* __restrict__ size) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < S; v += (int64_t)gridDim.x * blockDim.x) {
    const int32_t r = rank[v];
    size[v] = (r >= 0 && r < R) ? rmax[r] : 0.0;
  }
}

// ---- the eight counters of :602-640 in one pass
struct WlStuff {
  double v[WL_STUFF_MAX];
  int n;
};

__global__ __launch_bounds__(WL_BLOCK) void wl_label_stats_kernel(const double* __restrict__ weak_sem,
                                                                  const double* __restrict__ weak_ins,
                                                                  const double* __restrict__ sem_gt,
                                                                  const double* __restrict__ ins_gt, int64_t N,
                                                                  WlStuff stuff, unsigned long long* __restrict__ out) {
  int c[WL_NSTAT];
#pragma unroll
  for (int k = 0; k < WL_NSTAT; ++k) c[k] = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const double ws = weak_sem[i], wi = weak_ins[i], gs = sem_gt[i], gi = ins_gt[i];
    bool is_stuff = false;
    for (int j = 0; j < stuff.n; ++j) is_stuff |= ws == stuff.v[j];
    const bool has_sem = ws != -100.0, sem_ok = has_sem && ws == gs;
    const bool has_ins = wi != -100.0 && !is_stuff;
    c[0] += 1;
    c[1] += gs != -100.0;
    c[2] += has_sem;
    c[3] += sem_ok;
    c[4] += has_sem && is_stuff;
    c[5] += sem_ok && is_stuff;
    c[6] += has_ins;
    c[7] += has_ins && wi == gi;
  }
#pragma unroll
  for (int k = 0; k < WL_NSTAT; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c[k] += __shfl_xor(c[k], m);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < WL_NSTAT; ++k)
      if (c[k]) atomicAdd(out + k, (unsigned long long)c[k]);
  }
}

struct WlOccLayout {
  size_t coords, p2v, seen, counts2, vi, total;
  int64_t vi_bytes;
};

bool wl_occ_layout(int64_t N, WlOccLayout* L) {
  const int64_t vi_bytes = wsis_voxelize_idx_workspace_bytes(N);
  if (vi_bytes < 0) return false;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += align256(bytes);
    return o;
  };
  L->coords = take((size_t)N * 4 * sizeof(int64_t));
  L->p2v = take((size_t)N * sizeof(int32_t));
  L->seen = take((size_t)N * sizeof(int32_t));
  L->counts2 = take(2 * sizeof(int32_t));
  L->vi = take((size_t)vi_bytes);
  L->vi_bytes = vi_bytes;
  L->total = off + 256;
  return true;
}

}  // namespace

extern "C" {

int wsis_wl_sp_stats(const float* d_xyz, const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t S,
                     float* d_sum, int32_t* d_count, float* d_centre, void* stream) {
  WSIS_REQUIRE(N >= 0 && S >= 0, "negative size");
  WSIS_REQUIRE(N < ((int64_t)1 << 31), "N too large for the int32 CSR");
  if (S == 0) return WSIS_OK;
  WSIS_REQUIRE(d_offsets && d_sum && d_count && d_centre && (N == 0 || (d_xyz && d_perm)), "null pointer");
  const int64_t g = ceil_div(S, WL_WAVES);
  WSIS_REQUIRE(g <= 0x7fffffff, "S too large for one launch");
  hipLaunchKernelGGL(wl_sp_stats_kernel, dim3((unsigned)g), dim3(WL_BLOCK), 0, as_stream(stream), d_xyz, d_perm,
                     d_offsets, S, d_sum, d_count, d_centre);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_wl_neighbor_source(const int64_t* d_edges, int64_t E, const int64_t* d_sem, const int64_t* d_ins,
                            const int64_t* d_pred, const float* d_conf, double thr, int64_t S, int32_t* d_src,
                            void* stream) {
  WSIS_REQUIRE(E >= 0 && S >= 0, "negative size");
  WSIS_REQUIRE(S < ((int64_t)1 << 31), "S too large for int32 sources");
  if (S == 0) return WSIS_OK;
  WSIS_REQUIRE(d_src, "null pointer");
  hipStream_t st = as_stream(stream);
  WSIS_HIP_CHECK(hipMemsetAsync(d_src, 0xFF, (size_t)S * sizeof(int32_t), st));      // -1: no source
  if (E == 0) return WSIS_OK;
  WSIS_REQUIRE(d_edges && d_sem && d_ins && d_pred, "null pointer");
  hipLaunchKernelGGL(wl_neighbor_kernel, dim3(grid_for(E, WL_BLOCK)), dim3(WL_BLOCK), 0, st, d_edges, E, d_sem, d_ins,
                     d_pred, d_conf, thr, S, d_src);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_wl_apply_source(const int32_t* d_src, const int64_t* d_sem, const int64_t* d_ins, const double* d_off,
                         const float* d_centre, const int64_t* d_edges, int64_t E, int64_t S, int64_t* d_sem_out,
                         int64_t* d_ins_out, double* d_off_out, int64_t* d_is1ins, void* stream) {
  WSIS_REQUIRE(E >= 0 && S >= 0, "negative size");
  hipStream_t st = as_stream(stream);
  if (S > 0) {
    WSIS_REQUIRE(d_src && d_sem && d_ins && d_off && d_centre && d_sem_out && d_ins_out && d_off_out, "null pointer");
    WSIS_REQUIRE(d_sem_out != d_sem && d_ins_out != d_ins && d_off_out != d_off, "the outputs may not alias the inputs");
    hipLaunchKernelGGL(wl_apply_kernel, dim3(grid_for(S, WL_BLOCK)), dim3(WL_BLOCK), 0, st, d_src, d_sem, d_ins, d_off,
                       d_centre, S, d_sem_out, d_ins_out, d_off_out);
    WSIS_LAUNCH_CHECK();
  }
  if (E > 0) {
    WSIS_REQUIRE(d_edges && d_is1ins && d_ins_out, "null pointer");
    hipLaunchKernelGGL(wl_is1ins_kernel, dim3(grid_for(E, WL_BLOCK)), dim3(WL_BLOCK), 0, st, d_edges, E, d_ins_out, S,
                       d_is1ins);
    WSIS_LAUNCH_CHECK();
  }
  return WSIS_OK;
}

int wsis_wl_scene_assign(const int32_t* d_prior, int64_t P, const int64_t* d_sem, const int64_t* d_ins,
                         const double* d_off, const float* d_centre, const float* d_sum, const int32_t* d_count,
                         const int64_t* d_pred, const float* d_pred_off, double max_dist, int64_t S, int32_t* d_assigned,
                         double* d_dist, int64_t* d_sem_out, int64_t* d_ins_out, double* d_off_out, void* stream) {
  WSIS_REQUIRE(P >= 0 && S >= 0 && P <= S, "bad sizes");
  WSIS_REQUIRE(S < ((int64_t)1 << 31), "S too large for int32 indices");
  if (S == 0) return WSIS_OK;
  WSIS_REQUIRE(d_sem && d_ins && d_off && d_centre && d_sum && d_count && d_pred && d_pred_off && d_assigned && d_dist &&
                   d_sem_out && d_ins_out && d_off_out && (P == 0 || d_prior),
               "null pointer");
  WSIS_REQUIRE(d_sem_out != d_sem && d_ins_out != d_ins && d_off_out != d_off, "the outputs may not alias the inputs");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(wl_scene_search_kernel, dim3((unsigned)ceil_div(S, WL_SEARCH_BLOCK)), dim3(WL_SEARCH_BLOCK), 0, st,
                     d_prior, (int)P, d_sem, d_ins, d_off, d_centre, d_pred, d_pred_off, max_dist, S, d_assigned, d_dist,
                     d_sem_out, d_ins_out, d_off_out);
  WSIS_LAUNCH_CHECK();
  if (P > 0) {
    hipLaunchKernelGGL(wl_scene_gather_kernel, dim3((unsigned)ceil_div(P, WL_WAVES)), dim3(WL_BLOCK), 0, st, d_prior,
                       (int)P, d_assigned, d_sum, d_count, d_centre, d_sem, d_ins, S, d_sem_out, d_ins_out, d_off_out);
    WSIS_LAUNCH_CHECK();
  }
  return WSIS_OK;
}

int wsis_wl_point_labels(const int64_t* d_sp, int64_t N, const int64_t* d_sem, const int64_t* d_ins, double* d_weak_sem,
                         double* d_weak_ins, void* stream) {
  WSIS_REQUIRE(N >= 0, "N < 0");
  if (N == 0) return WSIS_OK;
  WSIS_REQUIRE(d_sp && d_sem && d_ins && d_weak_sem && d_weak_ins, "null pointer");
  hipLaunchKernelGGL(wl_point_labels_kernel, dim3(grid_for(N, WL_BLOCK)), dim3(WL_BLOCK), 0, as_stream(stream), d_sp, N,
                     d_sem, d_ins, d_weak_sem, d_weak_ins);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_wl_occupancy_workspace_bytes(int64_t N) {
  if (N < 0) return -1;
  WlOccLayout L;
  if (!wl_occ_layout(N, &L)) return -1;
  return (int64_t)L.total;
}

int wsis_wl_occupancy(const float* d_xyz, const int64_t* d_sp, const int32_t* d_rank_sp, int64_t N, int32_t R,
                      float scale, int64_t* d_vox_count, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(N >= 0 && R >= 0, "negative size");
  hipStream_t st = as_stream(stream);
  if (R > 0) {
    WSIS_REQUIRE(d_vox_count, "null pointer");
    WSIS_HIP_CHECK(hipMemsetAsync(d_vox_count, 0, (size_t)R * sizeof(int64_t), st));
  }
  if (N == 0 || R == 0) return WSIS_OK;
  WSIS_REQUIRE(d_xyz && d_sp && d_rank_sp && d_ws, "null pointer");
  WlOccLayout L;
  WSIS_REQUIRE(wl_occ_layout(N, &L), "workspace query failed");
  WSIS_REQUIRE((int64_t)L.total <= ws_bytes, "workspace too small");
  char* ws = static_cast<char*>(d_ws);
  int64_t* coords = reinterpret_cast<int64_t*>(ws + L.coords);
  int32_t* p2v = reinterpret_cast<int32_t*>(ws + L.p2v);
  int32_t* seen = reinterpret_cast<int32_t*>(ws + L.seen);
  int32_t* counts2 = reinterpret_cast<int32_t*>(ws + L.counts2);
  const int g = grid_for(N, WL_BLOCK);
  hipLaunchKernelGGL(wl_keys_kernel, dim3(g), dim3(WL_BLOCK), 0, st, d_xyz, d_sp, d_rank_sp, N, scale, coords);
  WSIS_LAUNCH_CHECK();
  const int rc = wsis_voxelize_idx_map(coords, N, p2v, counts2, ws + L.vi, L.vi_bytes, stream);
  if (rc != WSIS_OK) return rc;
  WSIS_HIP_CHECK(hipMemsetAsync(seen, 0, (size_t)N * sizeof(int32_t), st));
  hipLaunchKernelGGL(wl_voxel_count_kernel, dim3(g), dim3(WL_BLOCK), 0, st, p2v, coords, N, R, seen,
                     reinterpret_cast<unsigned long long*>(d_vox_count));
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_wl_instance_size(const double* d_off, const int32_t* d_rank, int64_t S, int32_t R, double* d_rmax,
                          double* d_size, void* stream) {
  WSIS_REQUIRE(S >= 0 && R >= 0, "negative size");
  hipStream_t st = as_stream(stream);
  if (R > 0) {
    WSIS_REQUIRE(d_rmax, "null pointer");
    WSIS_HIP_CHECK(hipMemsetAsync(d_rmax, 0, (size_t)R * sizeof(double), st));      // +0.0: the reference starts from 0
  }
  if (S == 0) return WSIS_OK;
  WSIS_REQUIRE(d_off && d_rank && d_size, "null pointer");
  const int g = grid_for(S, WL_BLOCK);
  if (R > 0) {
    hipLaunchKernelGGL(wl_size_max_kernel, dim3(g), dim3(WL_BLOCK), 0, st, d_off, d_rank, S, R,
                       reinterpret_cast<unsigned long long*>(d_rmax));
    WSIS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(wl_size_gather_kernel, dim3(g), dim3(WL_BLOCK), 0, st, d_rmax, d_rank, S, R, d_size);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_wl_label_stats(const double* d_weak_sem, const double* d_weak_ins, const double* d_sem_gt,
                        const double* d_ins_gt, int64_t N, const double* h_stuff, int32_t n_stuff, int64_t* d_counters,
                        void* stream) {
  WSIS_REQUIRE(N >= 0, "N < 0");
  WSIS_REQUIRE(n_stuff >= 0 && n_stuff <= WL_STUFF_MAX && (n_stuff == 0 || h_stuff), "0 <= n_stuff <= 8");
  WSIS_REQUIRE(d_counters, "null pointer");
  hipStream_t st = as_stream(stream);
  WSIS_HIP_CHECK(hipMemsetAsync(d_counters, 0, WL_NSTAT * sizeof(int64_t), st));
  if (N == 0) return WSIS_OK;
  WSIS_REQUIRE(d_weak_sem && d_weak_ins && d_sem_gt && d_ins_gt, "null pointer");
  WlStuff stuff;
  stuff.n = n_stuff;
  for (int j = 0; j < WL_STUFF_MAX; ++j) stuff.v[j] = j < n_stuff ? h_stuff[j] : 0.0;
  hipLaunchKernelGGL(wl_label_stats_kernel, dim3(grid_for(N, WL_BLOCK)), dim3(WL_BLOCK), 0, st, d_weak_sem, d_weak_ins,
                     d_sem_gt, d_ins_gt, N, stuff, reinterpret_cast<unsigned long long*>(d_counters));
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
