// l0 cut pursuit with L2 fidelity on the device: the solver libcp.cutpursuit of the reference
// (data/S3DIS/partition/cut-pursuit, mode 1, speed 4) that generate_SPG_superpoint calls at partition_S3DIS.py:110-111.
//
//   the arc structure of the input edges           API.h:959-974 (addDoubledge)                   wsis_cp_arcs
//   2-means start of the split                     CutPursuit_L2.h init_labels                    wsis_cp_kmeans
//   class centres, terminal differences            CutPursuit_L2.h compute_center, set_capacities wsis_cp_capacities
//   integer capacities of one flow                 (ours: the reference flows in fp32)            wsis_cp_quantize
//   max flow / min cut                             boost::boykov_kolmogorov_max_flow              wsis_cp_min_cut
//   active arcs, saturation, components            CutPursuit.h activate_edges, compute_connected_components
//                                                                                                 wsis_cp_activate
//   component values, borders, merge gains         CutPursuit.h compute_reduced_graph,
//                                                  CutPursuit_L2.h compute_value, compute_merge_gain
//                                                                                wsis_cp_values / _border_keys / _borders
//   the backward step                              CutPursuit.h merge                             wsis_cp_merge / _relabel
//   the energy                                     CutPursuit_L2.h compute_energy                 wsis_cp_energy
//
// Reproducibility: floating-point sums are fixed-order (strided partial sums and a tree per workgroup, or one sequential
// chain), never atomic; the flow works on integers, where atomic adds commute; maxima and minima go through integer
// atomics.  Two calls give the same bytes.  No workgroup waits for another one: every loop over launches is on the host,
// bounded, and ends in an error at its bound.
#include "common.h"

using namespace wsis;

namespace {

constexpr int CP_BLOCK = 256;
constexpr int CP_KM_BLOCK = 1024;                // the 2-means: one workgroup per component, and the first component is the graph
constexpr int CP_DMAX = 8;                       // feature dimensions (S3DIS: 7)
constexpr int32_t CP_INF = 0x3fffffff;           // height of a node the sink cannot be reached from
constexpr int CP_RELAX_SWEEPS = 8;               // relaxation sweeps of one global-relabel launch
constexpr int CP_RELAX_BATCH = 4;                // relabel launches between two read-backs
constexpr int CP_PUSH_SWEEPS = 16;               // push/relabel sweeps of one launch
constexpr int CP_PUSH_LAUNCHES = 4;              // push launches of one round (between two global relabels)
constexpr int CP_SCAN_BLOCK = 1024;
constexpr int CP_ENERGY_GRID = 256;

inline size_t cp_align(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ __forceinline__ int32_t ld_i32(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_i32(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ long long ld_i64(const long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sum over the workgroup of N threads in a fixed tree; every thread gets the result
template <int N = CP_BLOCK>
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = N / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ uint32_t cp_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// the random stream: a hash of (seed, main iteration, restart, smallest node of the component, draw)
__device__ __forceinline__ uint32_t cp_hash(uint32_t seed, uint32_t iter, uint32_t restart, uint32_t root, uint32_t draw) {
  uint32_t h = cp_mix(seed ^ 0x9e3779b9u);
  h = cp_mix(h + iter);
  h = cp_mix(h + restart);
  h = cp_mix(h + root);
  return cp_mix(h + draw);
}

__device__ __forceinline__ double cp_dist2(const float* __restrict__ x, const double* k, int D) {
  double s = 0.0;
  for (int d = 0; d < D; ++d) {
    const double t = (double)x[d] - k[d];
    s += t * t;
  }
  return s;
}

// ---------------------------------------------------------------------------------------------------------- arcs
__global__ __launch_bounds__(CP_BLOCK) void cp_arc_inv_kernel(const int32_t* __restrict__ perm, int64_t A,
                                                              int32_t* __restrict__ inv) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < A; p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t a = perm[p];
    if (a >= 0 && a < A) inv[a] = (int32_t)p;
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_arc_fill_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                                                               int64_t E, const int32_t* __restrict__ perm,
                                                               const int32_t* __restrict__ inv, int32_t* __restrict__ head,
                                                               int32_t* __restrict__ rev, int32_t* __restrict__ edge) {
  const int64_t A = 2 * E;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < A; p += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = perm[p];
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    const int64_t e = a < E ? a : a - E;
    head[p] = a < E ? tgt[e] : src[e];
    rev[p] = inv[a < E ? a + E : a - E];
    edge[p] = (int32_t)e;
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_arc_tails_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                                                                int64_t E, int64_t* __restrict__ tails) {
  for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < 2 * E; a += (int64_t)gridDim.x * blockDim.x)
    tails[a] = a < E ? src[a] : tgt[a - E];
}

// -------------------------------------------------------------------------------------------------------- 2-means
// one workgroup per component: all restarts and iterations of its 2-means.  label[v] = 1: the class whose mean is
// kernel 0 after the update (the reference's potential_label)
__global__ __launch_bounds__(CP_KM_BLOCK) void cp_kmeans_kernel(const float* __restrict__ f, int D,
                                                             const int32_t* __restrict__ off, const int32_t* __restrict__ nodes,
                                                             const uint8_t* __restrict__ sat, int64_t C, uint32_t seed,
                                                             uint32_t iter, int restarts, int kiters,
                                                             uint8_t* __restrict__ label, uint8_t* __restrict__ pot) {
  __shared__ double sh[CP_KM_BLOCK];
  __shared__ int found;
  const int t = threadIdx.x;
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    const int b = off[c], n = off[c + 1] - b;
    if (sat[c] || n <= 1) {
      for (int i = t; i < n; i += CP_KM_BLOCK) label[nodes[b + i]] = 0;
      continue;
    }
    const uint32_t root = (uint32_t)nodes[b];
    double best = __longlong_as_double(0x7ff0000000000000ll);
    for (int r = 0; r < restarts; ++r) {
      double k0[CP_DMAX], k1[CP_DMAX];
      const int first = (int)(cp_hash(seed, iter, (uint32_t)r, root, 0u) % (uint32_t)n);
      for (int d = 0; d < D; ++d) k0[d] = (double)f[(int64_t)nodes[b + first] * D + d];
      double part = 0.0;
      for (int i = t; i < n; i += CP_KM_BLOCK) part += cp_dist2(f + (int64_t)nodes[b + i] * D, k0, D);
      const double total = block_sum<CP_KM_BLOCK>(part, sh);
      const double thresh = total * ((double)cp_hash(seed, iter, (uint32_t)r, root, 1u) * (1.0 / 4294967296.0));
      // the second kernel: the first node, in the component's order, whose running sum exceeds thresh (else node 0)
      if (t == 0) found = 0x7fffffff;
      __syncthreads();
      double carry = 0.0;
      for (int base = 0; base < n; base += CP_KM_BLOCK) {
        const int i = base + t;
        sh[t] = i < n ? cp_dist2(f + (int64_t)nodes[b + i] * D, k0, D) : 0.0;
        __syncthreads();
        for (int s = 1; s < CP_KM_BLOCK; s <<= 1) {
          const double add = t >= s ? sh[t - s] : 0.0;
          __syncthreads();
          sh[t] += add;
          __syncthreads();
        }
        if (i < n && carry + sh[t] > thresh) atomicMin(&found, i);
        const double tile = sh[CP_KM_BLOCK - 1];
        __syncthreads();
        carry += tile;
        if (found != 0x7fffffff) break;
      }
      const int second = found == 0x7fffffff ? 0 : found;
      __syncthreads();
      for (int d = 0; d < D; ++d) k1[d] = (double)f[(int64_t)nodes[b + second] * D + d];
      for (int it = 0; it < kiters; ++it) {
        double s0[CP_DMAX], s1[CP_DMAX], n0 = 0.0, n1 = 0.0;
        for (int d = 0; d < D; ++d) s0[d] = s1[d] = 0.0;
        for (int i = t; i < n; i += CP_KM_BLOCK) {
          const int v = nodes[b + i];
          const float* x = f + (int64_t)v * D;
          const bool l = cp_dist2(x, k0, D) > cp_dist2(x, k1, D);
          pot[v] = l ? 1 : 0;
          if (l) {
            n0 += 1.0;
            for (int d = 0; d < D; ++d) s0[d] += (double)x[d];
          } else {
            n1 += 1.0;
            for (int d = 0; d < D; ++d) s1[d] += (double)x[d];
          }
        }
        n0 = block_sum<CP_KM_BLOCK>(n0, sh);
        n1 = block_sum<CP_KM_BLOCK>(n1, sh);
        if (n0 == 0.0 || n1 == 0.0) break;       // an empty class: the kernels stay
        for (int d = 0; d < D; ++d) {
          k0[d] = block_sum<CP_KM_BLOCK>(s0[d], sh) / n0;
          k1[d] = block_sum<CP_KM_BLOCK>(s1[d], sh) / n1;
        }
      }
      part = 0.0;
      for (int i = t; i < n; i += CP_KM_BLOCK) {
        const int v = nodes[b + i];
        part += cp_dist2(f + (int64_t)v * D, pot[v] ? k0 : k1, D);
      }
      const double energy = block_sum<CP_KM_BLOCK>(part, sh);
      if (energy < best) {
        best = energy;
        for (int i = t; i < n; i += CP_KM_BLOCK) {
          const int v = nodes[b + i];
          label[v] = pot[v];
        }
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------- capacities
// one workgroup per component: the means of the two label classes; an empty class saturates the component.
// term[v] = cost_B - cost_notB of set_capacities (> 0: capacity from the source, < 0: to the sink)
__global__ __launch_bounds__(CP_BLOCK) void cp_capacities_kernel(const float* __restrict__ f, int D,
                                                                 const int32_t* __restrict__ off, const int32_t* __restrict__ nodes,
                                                                 int64_t C, const uint8_t* __restrict__ label,
                                                                 uint8_t* __restrict__ sat, double* __restrict__ centres,
                                                                 double* __restrict__ term) {
  __shared__ double sh[CP_BLOCK];
  const int t = threadIdx.x;
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    const int b = off[c], n = off[c + 1] - b;
    double c0[CP_DMAX], c1[CP_DMAX], n0 = 0.0, n1 = 0.0;
    for (int d = 0; d < D; ++d) c0[d] = c1[d] = 0.0;
    bool saturated = sat[c] != 0;
    if (!saturated) {
      for (int i = t; i < n; i += CP_BLOCK) {
        const int v = nodes[b + i];
        const float* x = f + (int64_t)v * D;
        if (label[v]) {
          n0 += 1.0;
          for (int d = 0; d < D; ++d) c0[d] += (double)x[d];
        } else {
          n1 += 1.0;
          for (int d = 0; d < D; ++d) c1[d] += (double)x[d];
        }
      }
      n0 = block_sum(n0, sh);
      n1 = block_sum(n1, sh);
      saturated = n0 == 0.0 || n1 == 0.0;
      if (!saturated)
        for (int d = 0; d < D; ++d) {
          c0[d] = block_sum(c0[d], sh) / n0;
          c1[d] = block_sum(c1[d], sh) / n1;
        }
    }
    if (saturated) {
      if (t == 0) sat[c] = 1;
      for (int d = t; d < 2 * D; d += CP_BLOCK) centres[c * 2 * D + d] = 0.0;
      for (int i = t; i < n; i += CP_BLOCK) term[nodes[b + i]] = 0.0;
      continue;
    }
    if (t == 0)
      for (int d = 0; d < D; ++d) {
        centres[c * 2 * D + d] = c0[d];
        centres[c * 2 * D + D + d] = c1[d];
      }
    for (int i = t; i < n; i += CP_BLOCK) {
      const int v = nodes[b + i];
      const float* x = f + (int64_t)v * D;
      double cb = 0.0, cn = 0.0;
      for (int d = 0; d < D; ++d) {
        cb += 0.5 * (c0[d] * c0[d] - 2.0 * (c0[d] * (double)x[d]));
        cn += 0.5 * (c1[d] * c1[d] - 2.0 * (c1[d] * (double)x[d]));
      }
      term[v] = cb - cn;
    }
  }
}

// the largest capacity of one flow, as the bits of a non-negative double (monotone as an integer)
__global__ __launch_bounds__(CP_BLOCK) void cp_capmax_kernel(const double* __restrict__ term, int64_t V,
                                                             const float* __restrict__ w, const uint8_t* __restrict__ active,
                                                             int64_t E, double lam, unsigned long long* __restrict__ mx) {
  unsigned long long m = 0;
  const int64_t n = V > E ? V : E;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < V) {
      const unsigned long long u = (unsigned long long)__double_as_longlong(fabs(term[i]));
      m = u > m ? u : m;
    }
    if (i < E && !(active && active[i])) {
      const unsigned long long u = (unsigned long long)__double_as_longlong(fabs(lam * (double)w[i]));
      m = u > m ? u : m;
    }
  }
  if (m) atomicMax(mx, m);
}
// scale = 2^(ex - 30) with max < 2^ex: a capacity fits 31 bits, the excess of 2^32 nodes fits int64; max = 0: scale 1
__global__ void cp_scale_kernel(const unsigned long long* __restrict__ mx, double* __restrict__ scale) {
  const double m = __longlong_as_double((long long)*mx);
  int ex = 0;
  if (m > 0.0) {
    frexp(m, &ex);
    *scale = ldexp(1.0, ex - 30);
  } else {
    *scale = 1.0;
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_quantize_kernel(const double* __restrict__ term, int64_t V,
                                                               const float* __restrict__ w, const uint8_t* __restrict__ active,
                                                               int64_t E, double lam, const int32_t* __restrict__ arc_edge,
                                                               int64_t A, const double* __restrict__ scale,
                                                               int32_t* __restrict__ src_cap, int32_t* __restrict__ snk_cap,
                                                               int32_t* __restrict__ arc_cap) {
  const double s = *scale;
  const int64_t n = V > A ? V : A;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < V) {
      const double x = term[i];
      src_cap[i] = x > 0.0 ? (int32_t)llrint(x / s) : 0;
      snk_cap[i] = x < 0.0 ? (int32_t)llrint(-x / s) : 0;
    }
    if (i < A) {
      int64_t e = arc_edge[i];
      e = e < 0 ? 0 : (e >= E ? E - 1 : e);
      arc_cap[i] = (active && active[e]) ? 0 : (int32_t)llrint(fabs(lam * (double)w[e]) / s);
    }
  }
}

// -------------------------------------------------------------------------------------------------------- min cut
// The terminals are implicit.  ex[v] = src_cap - snk_cap + net inflow: > 0 an excess to push on, < 0 what the arc to
// the sink can still take (such a node has height 0).  res[a]: residual capacity of arc a.
__global__ __launch_bounds__(CP_BLOCK) void cp_flow_init_kernel(const int32_t* __restrict__ src_cap,
                                                                const int32_t* __restrict__ snk_cap, int64_t V,
                                                                const int32_t* __restrict__ arc_off,
                                                                const int32_t* __restrict__ arc_head,
                                                                const int32_t* __restrict__ arc_cap, long long* __restrict__ ex,
                                                                int32_t* __restrict__ res) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    ex[v] = (long long)src_cap[v] - (long long)snk_cap[v];
    for (int a = arc_off[v]; a < arc_off[v + 1]; ++a) res[a] = arc_head[a] == v ? 0 : (arc_cap[a] > 0 ? arc_cap[a] : 0);
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_height_init_kernel(const long long* __restrict__ ex, int64_t V,
                                                                  int32_t* __restrict__ h) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x)
    h[v] = ex[v] < 0 ? 0 : CP_INF;
}
// global relabel: heights fall from CP_INF to the exact residual distance to a node with ex < 0; updates in place are
// monotone, so any interleaving ends at the same fixed point.  *counters != 0: something changed in this launch
__global__ __launch_bounds__(CP_BLOCK) void cp_relax_kernel(const long long* __restrict__ ex, int64_t V, int64_t A,
                                                            const int32_t* __restrict__ arc_off,
                                                            const int32_t* __restrict__ arc_head, const int32_t* __restrict__ res,
                                                            int32_t* __restrict__ h, int32_t* __restrict__ counters) {
  bool changed = false;
  for (int sweep = 0; sweep < CP_RELAX_SWEEPS; ++sweep) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
      if (ex[v] < 0) continue;
      int32_t m = CP_INF;
      for (int a = arc_off[v]; a < arc_off[v + 1]; ++a) {
        if (res[a] <= 0) continue;
        const int32_t u = arc_head[a];
        if ((uint32_t)u >= (uint32_t)V) continue;
        const int32_t hu = ld_i32(h + u);
        m = hu < m ? hu : m;
      }
      if (m + 1 < ld_i32(h + v)) {
        st_i32(h + v, m + 1);
        changed = true;
      }
    }
  }
  if (changed) atomicOr(counters, 1);
}
__global__ __launch_bounds__(CP_BLOCK) void cp_active_kernel(const long long* __restrict__ ex, const int32_t* __restrict__ h,
                                                             int64_t V, int32_t* __restrict__ counters) {
  int n = 0;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x)
    n += (ex[v] > 0 && h[v] < CP_INF) ? 1 : 0;
  if (n) atomicAdd(counters, n);
}
// asynchronous push-relabel (Hong and He 2011): the owner of node u alone lowers ex[u] and the residuals of u's arcs and
// alone writes h[u]; everybody else only raises them, so the amounts below are never overdrawn.  A push goes to the
// lowest residual neighbour and only downhill; a node with no residual neighbour below CP_INF leaves the game.
__global__ __launch_bounds__(CP_BLOCK) void cp_push_kernel(long long* __restrict__ ex, int64_t V,
                                                           const int32_t* __restrict__ arc_off,
                                                           const int32_t* __restrict__ arc_head, const int32_t* __restrict__ arc_rev,
                                                           int64_t A, int32_t* __restrict__ res, int32_t* __restrict__ h) {
  for (int sweep = 0; sweep < CP_PUSH_SWEEPS; ++sweep) {
    for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < V; u += (int64_t)gridDim.x * blockDim.x) {
      const long long e = ld_i64(ex + u);
      const int32_t hu = ld_i32(h + u);
      if (e <= 0 || hu >= CP_INF) continue;
      int32_t hmin = CP_INF, amin = -1;
      for (int a = arc_off[u]; a < arc_off[u + 1]; ++a) {
        if (ld_i32(res + a) <= 0) continue;
        const int32_t v = arc_head[a];
        if ((uint32_t)v >= (uint32_t)V) continue;
        const int32_t hv = ld_i32(h + v);
        if (hv < hmin) {
          hmin = hv;
          amin = a;
        }
      }
      if (amin < 0) {
        st_i32(h + u, CP_INF);
      } else if (hu > hmin) {
        const int32_t r = ld_i32(res + amin);
        const int32_t d = e < (long long)r ? (int32_t)e : r;
        const int32_t back = arc_rev[amin];
        atomicSub(res + amin, d);
        if ((uint32_t)back < (uint32_t)A) atomicAdd(res + back, d);
        atomicAdd(reinterpret_cast<unsigned long long*>(ex + u), (unsigned long long)(-(long long)d));
        atomicAdd(reinterpret_cast<unsigned long long*>(ex + arc_head[amin]), (unsigned long long)d);
      } else {
        st_i32(h + u, hmin + 1 > V ? CP_INF : hmin + 1);
      }
    }
  }
}
// sink_side[v] = the sink is reachable from v in the residual graph; the cut value from the partition
__global__ __launch_bounds__(CP_BLOCK) void cp_cut_kernel(const int32_t* __restrict__ h, int64_t V,
                                                          const int32_t* __restrict__ src_cap, const int32_t* __restrict__ snk_cap,
                                                          const int32_t* __restrict__ arc_off, const int32_t* __restrict__ arc_head,
                                                          const int32_t* __restrict__ arc_cap, uint8_t* __restrict__ sink_side,
                                                          unsigned long long* __restrict__ cut) {
  unsigned long long s = 0;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const bool sink = h[v] < CP_INF;
    sink_side[v] = sink ? 1 : 0;
    if (sink) {
      s += (unsigned long long)src_cap[v];
    } else {
      s += (unsigned long long)snk_cap[v];
      for (int a = arc_off[v]; a < arc_off[v + 1]; ++a) {
        const int32_t u = arc_head[a];
        if ((uint32_t)u >= (uint32_t)V || u == v) continue;
        if (h[u] < CP_INF && arc_cap[a] > 0) s += (unsigned long long)arc_cap[a];
      }
    }
  }
  if (s) atomicAdd(cut, s);
}

// ------------------------------------------------------------------------------------------- activation, components
__global__ __launch_bounds__(CP_BLOCK) void cp_saturate_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ nodes,
                                                               int64_t C, const uint8_t* __restrict__ label,
                                                               uint8_t* __restrict__ sat) {
  __shared__ int cnt;
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const int b = off[c], n = off[c + 1] - b;
    if (!sat[c]) {
      int k = 0;
      for (int i = threadIdx.x; i < n; i += CP_BLOCK) k += label[nodes[b + i]] ? 1 : 0;
      if (k) atomicAdd(&cnt, k);
    }
    __syncthreads();
    if (threadIdx.x == 0 && !sat[c] && (cnt == 0 || cnt == n)) sat[c] = 1;
    __syncthreads();
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_activate_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                                                               int64_t E, const uint8_t* __restrict__ label,
                                                               uint8_t* __restrict__ active) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x)
    if (label[src[e]] != label[tgt[e]]) active[e] = 1;
}
__global__ __launch_bounds__(CP_BLOCK) void cp_iota_kernel(int32_t* __restrict__ p, int64_t V) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) p[v] = (int32_t)v;
}
// parents only ever fall and never point upwards: a walk to the root ends
__device__ __forceinline__ int32_t cp_find(const int32_t* parent, int32_t v) {
  int32_t p = ld_i32(parent + v);
  while (p != v) {
    v = p;
    p = ld_i32(parent + v);
  }
  return v;
}
__global__ __launch_bounds__(CP_BLOCK) void cp_hook_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                                                           int64_t E, const uint8_t* __restrict__ active,
                                                           int32_t* __restrict__ parent, int32_t* __restrict__ changed) {
  bool any = false;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    if (active[e] || src[e] == tgt[e]) continue;
    const int32_t ru = cp_find(parent, src[e]), rv = cp_find(parent, tgt[e]);
    if (ru == rv) continue;
    atomicMin(parent + (ru > rv ? ru : rv), ru > rv ? rv : ru);
    any = true;
  }
  if (any) atomicOr(changed, 1);
}
__global__ __launch_bounds__(CP_BLOCK) void cp_compress_kernel(int32_t* __restrict__ parent, int64_t V) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x)
    st_i32(parent + v, cp_find(parent, (int32_t)v));
}
__global__ __launch_bounds__(CP_BLOCK) void cp_rootflag_kernel(const int32_t* __restrict__ parent, int64_t V,
                                                               int32_t* __restrict__ flag) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x)
    flag[v] = parent[v] == v ? 1 : 0;
}
// exclusive prefix sum of n flags in place, in one workgroup; *total = their sum
__global__ __launch_bounds__(CP_SCAN_BLOCK) void cp_scan_kernel(int32_t* __restrict__ flag, int64_t n, int32_t* __restrict__ total) {
  __shared__ int32_t sh[CP_SCAN_BLOCK];
  const int t = threadIdx.x;
  const int64_t chunk = (n + CP_SCAN_BLOCK - 1) / CP_SCAN_BLOCK;
  const int64_t lo = t * chunk, hi = lo + chunk < n ? lo + chunk : n;
  int32_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += flag[i];
  sh[t] = s;
  __syncthreads();
  for (int k = 1; k < CP_SCAN_BLOCK; k <<= 1) {
    const int32_t add = t >= k ? sh[t - k] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  int32_t run = sh[t] - s;
  for (int64_t i = lo; i < hi; ++i) {
    const int32_t x = flag[i];
    flag[i] = run;
    run += x;
  }
  if (t == CP_SCAN_BLOCK - 1) *total = sh[t];
}
__global__ __launch_bounds__(CP_BLOCK) void cp_newcomp_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ rank,
                                                              int64_t V, const int32_t* __restrict__ comp_old,
                                                              const uint8_t* __restrict__ sat_old, int64_t C,
                                                              int32_t* __restrict__ comp_new, uint8_t* __restrict__ sat_new) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const int32_t r = parent[v];
    comp_new[v] = rank[r];
    if (r == v) {
      const int32_t c = comp_old[v];
      sat_new[rank[v]] = ((uint32_t)c < (uint32_t)C) ? sat_old[c] : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- reduced graph
__global__ __launch_bounds__(CP_BLOCK) void cp_values_kernel(const float* __restrict__ f, int D, const int32_t* __restrict__ off,
                                                             const int32_t* __restrict__ nodes, int64_t C,
                                                             double* __restrict__ mean, double* __restrict__ weight) {
  __shared__ double sh[CP_BLOCK];
  const int t = threadIdx.x;
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    const int b = off[c], n = off[c + 1] - b;
    double s[CP_DMAX];
    for (int d = 0; d < D; ++d) s[d] = 0.0;
    for (int i = t; i < n; i += CP_BLOCK) {
      const float* x = f + (int64_t)nodes[b + i] * D;
      for (int d = 0; d < D; ++d) s[d] += (double)x[d];
    }
    for (int d = 0; d < D; ++d) {
      const double r = block_sum(s[d], sh);
      if (t == 0) mean[c * D + d] = r / (double)n;
    }
    if (t == 0) weight[c] = (double)n;
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_border_keys_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                                                                  const int32_t* __restrict__ comp, int64_t E, int64_t C,
                                                                  int64_t* __restrict__ keys) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = comp[src[e]], b = comp[tgt[e]];
    keys[e] = a == b ? 0x7fffffffffffffffll : (a < b ? a * C + b : b * C + a);
  }
}
// one thread per border: the weights of its edges in ascending edge order, then the gain of the merge
__global__ __launch_bounds__(CP_BLOCK) void cp_borders_kernel(const int64_t* __restrict__ ukeys, const int64_t* __restrict__ boff,
                                                              const int64_t* __restrict__ order, const float* __restrict__ w,
                                                              int64_t E, const double* __restrict__ mean,
                                                              const double* __restrict__ weight, int D, double lam, int64_t B,
                                                              int64_t C, int32_t* __restrict__ ba, int32_t* __restrict__ bb,
                                                              double* __restrict__ bw, double* __restrict__ gain) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = ukeys[i];
    int64_t a = k / C, b = k % C;
    a = a < 0 ? 0 : (a >= C ? C - 1 : a);
    b = b < 0 ? 0 : (b >= C ? C - 1 : b);
    double s = 0.0;
    for (int64_t j = boff[i]; j < boff[i + 1]; ++j) {
      const int64_t e = order[j];
      if (e >= 0 && e < E) s += (double)w[e];
    }
    const double w1 = weight[a], w2 = weight[b];
    double g = 0.0;
    for (int d = 0; d < D; ++d) {
      const double v1 = mean[a * D + d], v2 = mean[b * D + d];
      const double mv = (w1 * v1 + w2 * v2) / (w1 + w2);
      g += 0.5 * (mv * mv * (w1 + w2) - v1 * v1 * w1 - v2 * v2 * w2);
    }
    ba[i] = (int32_t)a;
    bb[i] = (int32_t)b;
    bw[i] = s;
    gain[i] = g + s * lam;
  }
}

// ------------------------------------------------------------------------------------------------------------ merge
// greedy matching by (gain descending, border index ascending) as rounds of locally dominant borders
__device__ __forceinline__ bool cp_live(const int32_t* ba, const int32_t* bb, const double* gain, const uint8_t* matched,
                                        int64_t i) {
  return gain[i] > 0.0 && !matched[ba[i]] && !matched[bb[i]];
}
__global__ __launch_bounds__(CP_BLOCK) void cp_merge_reset_kernel(unsigned long long* __restrict__ best_gain,
                                                                  int32_t* __restrict__ best_idx, int64_t C) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < C; c += (int64_t)gridDim.x * blockDim.x) {
    best_gain[c] = 0;
    best_idx[c] = 0x7fffffff;
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_merge_gain_kernel(const int32_t* __restrict__ ba, const int32_t* __restrict__ bb,
                                                                 const double* __restrict__ gain, const uint8_t* __restrict__ matched,
                                                                 int64_t B, unsigned long long* __restrict__ best_gain) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
    if (!cp_live(ba, bb, gain, matched, i)) continue;
    const unsigned long long g = (unsigned long long)__double_as_longlong(gain[i]);
    atomicMax(best_gain + ba[i], g);
    atomicMax(best_gain + bb[i], g);
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_merge_idx_kernel(const int32_t* __restrict__ ba, const int32_t* __restrict__ bb,
                                                                const double* __restrict__ gain, const uint8_t* __restrict__ matched,
                                                                int64_t B, const unsigned long long* __restrict__ best_gain,
                                                                int32_t* __restrict__ best_idx) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
    if (!cp_live(ba, bb, gain, matched, i)) continue;
    const unsigned long long g = (unsigned long long)__double_as_longlong(gain[i]);
    if (best_gain[ba[i]] == g) atomicMin(best_idx + ba[i], (int32_t)i);
    if (best_gain[bb[i]] == g) atomicMin(best_idx + bb[i], (int32_t)i);
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_merge_take_kernel(const int32_t* __restrict__ ba, const int32_t* __restrict__ bb,
                                                                 const double* __restrict__ gain, int64_t B,
                                                                 const int32_t* __restrict__ best_idx, uint8_t* __restrict__ matched_next,
                                                                 uint8_t* __restrict__ taken, int32_t* __restrict__ map,
                                                                 int32_t* __restrict__ took) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
    if (!(gain[i] > 0.0) || taken[i]) continue;
    if (best_idx[ba[i]] == (int32_t)i && best_idx[bb[i]] == (int32_t)i) {
      taken[i] = 1;
      matched_next[ba[i]] = 1;
      matched_next[bb[i]] = 1;
      map[bb[i]] = ba[i];
      atomicOr(took, 1);
    }
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_keepflag_kernel(const int32_t* __restrict__ map, int64_t C, int32_t* __restrict__ flag,
                                                               uint8_t* __restrict__ merged) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < C; c += (int64_t)gridDim.x * blockDim.x) {
    const int32_t m = map[c];
    flag[c] = m == c ? 1 : 0;
    if (m != c && (uint32_t)m < (uint32_t)C) merged[m] = 1;
  }
}
__global__ __launch_bounds__(CP_BLOCK) void cp_relabel_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ newid,
                                                              const uint8_t* __restrict__ merged, int64_t C,
                                                              const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                                                              int64_t E, const int32_t* __restrict__ comp, int64_t V,
                                                              const uint8_t* __restrict__ sat, uint8_t* __restrict__ active,
                                                              int32_t* __restrict__ comp_new, uint8_t* __restrict__ sat_new) {
  const int64_t n = E > V ? E : V;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < E) {
      const int32_t cu = comp[src[i]], cv = comp[tgt[i]];
      if (cu != cv && map[cu] == map[cv]) active[i] = 0;
    }
    if (i < V) comp_new[i] = newid[map[comp[i]]];
    if (i < C && map[i] == (int32_t)i) sat_new[newid[i]] = (sat[i] && !merged[i]) ? 1 : 0;
  }
}

// ----------------------------------------------------------------------------------------------------------- energy
// part[g] = (fidelity, penalty without lambda, nodes of saturated components) of workgroup g; then one fixed-order sum
__global__ __launch_bounds__(CP_BLOCK) void cp_energy_part_kernel(const float* __restrict__ f, int D, const int32_t* __restrict__ comp,
                                                                  const double* __restrict__ mean, int64_t V, int64_t C,
                                                                  const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                                                                  const float* __restrict__ w, int64_t E,
                                                                  const uint8_t* __restrict__ sat, double* __restrict__ part) {
  __shared__ double sh[CP_BLOCK];
  double fid = 0.0, pen = 0.0, ns = 0.0;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    int64_t c = comp[v];
    c = c < 0 ? 0 : (c >= C ? C - 1 : c);
    fid += cp_dist2(f + v * D, mean + c * D, D);
    ns += sat[c] ? 1.0 : 0.0;
  }
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x)
    if (comp[src[e]] != comp[tgt[e]]) pen += (double)w[e];
  fid = block_sum(fid, sh);
  pen = block_sum(pen, sh);
  ns = block_sum(ns, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x * 3 + 0] = fid;
    part[blockIdx.x * 3 + 1] = pen;
    part[blockIdx.x * 3 + 2] = ns;
  }
}
__global__ void cp_energy_finish_kernel(const double* __restrict__ part, int G, double lam, double* __restrict__ out) {
  double fid = 0.0, pen = 0.0, ns = 0.0;
  for (int g = 0; g < G; ++g) {
    fid += part[g * 3 + 0];
    pen += part[g * 3 + 1];
    ns += part[g * 3 + 2];
  }
  out[0] = 0.5 * fid;
  out[1] = lam * pen;
  out[2] = ns;
}

inline int comp_grid(int64_t C) {
  int64_t g = C < 1 ? 1 : C;
  return (int)(g > 256 * 8 ? 256 * 8 : g);
}

struct FlowLayout {
  size_t ex, h, res, counters, total;
};
inline FlowLayout flow_layout(int64_t V, int64_t A) {
  FlowLayout l;
  size_t o = 0;
  l.ex = o;
  o += cp_align((size_t)V * 8);
  l.h = o;
  o += cp_align((size_t)V * 4);
  l.res = o;
  o += cp_align((size_t)(A > 0 ? A : 1) * 4);
  l.counters = o;
  o += 256;
  l.total = o;
  return l;
}

}  // namespace

extern "C" {

int wsis_cp_arc_tails(const int32_t* d_source, const int32_t* d_target, int64_t E, int64_t* d_tails, void* stream) {
  WSIS_REQUIRE(E >= 0 && E < ((int64_t)1 << 29), "0 <= E < 2^29");
  if (E == 0) return WSIS_OK;
  WSIS_REQUIRE(d_source && d_target && d_tails, "null pointer");
  hipLaunchKernelGGL(cp_arc_tails_kernel, dim3(grid_for(2 * E, CP_BLOCK)), dim3(CP_BLOCK), 0, as_stream(stream), d_source,
                     d_target, E, d_tails);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_cp_arcs_workspace_bytes(int64_t E) {
  if (E < 0 || E >= ((int64_t)1 << 29)) return -1;
  return (int64_t)cp_align((size_t)(2 * E + 1) * 4);
}

int wsis_cp_arcs(const int32_t* d_source, const int32_t* d_target, int64_t E, const int32_t* d_perm, int32_t* d_arc_head,
                 int32_t* d_arc_rev, int32_t* d_arc_edge, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(E >= 0 && E < ((int64_t)1 << 29), "0 <= E < 2^29");
  if (E == 0) return WSIS_OK;
  WSIS_REQUIRE(d_source && d_target && d_perm && d_arc_head && d_arc_rev && d_arc_edge && d_ws, "null pointer");
  WSIS_REQUIRE(ws_bytes >= wsis_cp_arcs_workspace_bytes(E), "workspace too small");
  hipStream_t st = as_stream(stream);
  int32_t* inv = static_cast<int32_t*>(d_ws);
  hipLaunchKernelGGL(cp_arc_inv_kernel, dim3(grid_for(2 * E, CP_BLOCK)), dim3(CP_BLOCK), 0, st, d_perm, 2 * E, inv);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_arc_fill_kernel, dim3(grid_for(2 * E, CP_BLOCK)), dim3(CP_BLOCK), 0, st, d_source, d_target, E, d_perm,
                     inv, d_arc_head, d_arc_rev, d_arc_edge);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_cp_kmeans_workspace_bytes(int64_t V) { return V < 1 ? -1 : (int64_t)cp_align((size_t)V); }

int wsis_cp_kmeans(const float* d_features, int32_t D, const int32_t* d_comp_off, const int32_t* d_comp_nodes,
                   const uint8_t* d_sat, int64_t C, int64_t V, uint32_t seed, uint32_t iteration, int32_t restarts,
                   int32_t kmeans_ite, uint8_t* d_label, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(V >= 1 && C >= 1 && C <= V && V < ((int64_t)1 << 30), "1 <= C <= V < 2^30");
  WSIS_REQUIRE(D >= 1 && D <= CP_DMAX, "1 <= D <= 8");
  WSIS_REQUIRE(restarts >= 1 && kmeans_ite >= 1, "restarts, kmeans_ite >= 1");
  WSIS_REQUIRE(d_features && d_comp_off && d_comp_nodes && d_sat && d_label && d_ws, "null pointer");
  WSIS_REQUIRE(ws_bytes >= wsis_cp_kmeans_workspace_bytes(V), "workspace too small");
  hipLaunchKernelGGL(cp_kmeans_kernel, dim3(comp_grid(C)), dim3(CP_KM_BLOCK), 0, as_stream(stream), d_features, D, d_comp_off,
                     d_comp_nodes, d_sat, C, seed, iteration, restarts, kmeans_ite, d_label, static_cast<uint8_t*>(d_ws));
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_cp_capacities(const float* d_features, int32_t D, const int32_t* d_comp_off, const int32_t* d_comp_nodes, int64_t C,
                       int64_t V, const uint8_t* d_label, uint8_t* d_sat, double* d_centres, double* d_term, void* stream) {
  WSIS_REQUIRE(V >= 1 && C >= 1 && C <= V && V < ((int64_t)1 << 30), "1 <= C <= V < 2^30");
  WSIS_REQUIRE(D >= 1 && D <= CP_DMAX, "1 <= D <= 8");
  WSIS_REQUIRE(d_features && d_comp_off && d_comp_nodes && d_label && d_sat && d_centres && d_term, "null pointer");
  hipLaunchKernelGGL(cp_capacities_kernel, dim3(comp_grid(C)), dim3(CP_BLOCK), 0, as_stream(stream), d_features, D, d_comp_off,
                     d_comp_nodes, C, d_label, d_sat, d_centres, d_term);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_cp_quantize(const double* d_term, int64_t V, const float* d_edge_weight, const uint8_t* d_active, int64_t E, double lam,
                     const int32_t* d_arc_edge, int32_t* d_src_cap, int32_t* d_snk_cap, int32_t* d_arc_cap, double* d_scale2,
                     void* stream) {
  WSIS_REQUIRE(V >= 1 && V < ((int64_t)1 << 30) && E >= 0 && E < ((int64_t)1 << 29), "1 <= V < 2^30, 0 <= E < 2^29");
  WSIS_REQUIRE(lam >= 0.0 && lam <= 1.7976931348623157e308, "lambda must be finite and non-negative");
  WSIS_REQUIRE(d_term && d_src_cap && d_snk_cap && d_scale2, "null pointer");
  WSIS_REQUIRE(E == 0 || (d_edge_weight && d_arc_edge && d_arc_cap), "null pointer");
  hipStream_t st = as_stream(stream);
  unsigned long long* mx = reinterpret_cast<unsigned long long*>(d_scale2 + 1);
  WSIS_HIP_CHECK(hipMemsetAsync(mx, 0, 8, st));
  hipLaunchKernelGGL(cp_capmax_kernel, dim3(grid_for(V > E ? V : E, CP_BLOCK)), dim3(CP_BLOCK), 0, st, d_term, V, d_edge_weight,
                     d_active, E, lam, mx);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_scale_kernel, dim3(1), dim3(1), 0, st, mx, d_scale2);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_quantize_kernel, dim3(grid_for(V > 2 * E ? V : 2 * E, CP_BLOCK)), dim3(CP_BLOCK), 0, st, d_term, V,
                     d_edge_weight, d_active, E, lam, d_arc_edge, 2 * E, d_scale2, d_src_cap, d_snk_cap, d_arc_cap);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_cp_min_cut_workspace_bytes(int64_t V, int64_t A) {
  if (V < 1 || V >= ((int64_t)1 << 30) || A < 0 || A >= ((int64_t)1 << 30)) return -1;
  return (int64_t)flow_layout(V, A).total;
}

int wsis_cp_min_cut(const int32_t* d_src_cap, const int32_t* d_snk_cap, const int32_t* d_arc_off, const int32_t* d_arc_head,
                    const int32_t* d_arc_rev, const int32_t* d_arc_cap, int64_t V, int64_t A, int32_t max_rounds,
                    uint8_t* d_sink_side, int64_t* d_cut, int32_t* h_rounds, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(V >= 1 && V < ((int64_t)1 << 30) && A >= 0 && A < ((int64_t)1 << 30), "1 <= V < 2^30, 0 <= A < 2^30");
  WSIS_REQUIRE(max_rounds >= 1, "max_rounds >= 1");
  WSIS_REQUIRE(d_src_cap && d_snk_cap && d_arc_off && d_sink_side && d_cut && h_rounds && d_ws, "null pointer");
  WSIS_REQUIRE(A == 0 || (d_arc_head && d_arc_rev && d_arc_cap), "null pointer");
  WSIS_REQUIRE(ws_bytes >= wsis_cp_min_cut_workspace_bytes(V, A), "workspace too small");
  hipStream_t st = as_stream(stream);
  const FlowLayout l = flow_layout(V, A);
  char* ws = static_cast<char*>(d_ws);
  long long* ex = reinterpret_cast<long long*>(ws + l.ex);
  int32_t* h = reinterpret_cast<int32_t*>(ws + l.h);
  int32_t* res = reinterpret_cast<int32_t*>(ws + l.res);
  int32_t* counters = reinterpret_cast<int32_t*>(ws + l.counters);
  const dim3 grid(grid_for(V, CP_BLOCK)), block(CP_BLOCK);
  hipLaunchKernelGGL(cp_flow_init_kernel, grid, block, 0, st, d_src_cap, d_snk_cap, V, d_arc_off, d_arc_head, d_arc_cap, ex, res);
  WSIS_LAUNCH_CHECK();
  int32_t rounds = 0;
  for (;;) {
    hipLaunchKernelGGL(cp_height_init_kernel, grid, block, 0, st, ex, V, h);
    WSIS_LAUNCH_CHECK();
    // counters[i] != 0: relabel launch i of the batch changed a height; counters[CP_RELAX_BATCH]: the active nodes.  A
    // launch that changed nothing saw constant heights in every one of its sweeps: the fixed point.  A sweep that changes
    // something fixes at least one more node's height: V sweeps at the most
    int32_t host[CP_RELAX_BATCH + 1];
    host[CP_RELAX_BATCH - 1] = 1;
    for (int64_t batch = 0; host[CP_RELAX_BATCH - 1]; ++batch) {
      if (batch * CP_RELAX_BATCH * CP_RELAX_SWEEPS > V + CP_RELAX_BATCH * CP_RELAX_SWEEPS)
        return fail(WSIS_ERR_OVERFLOW, "wsis_cp_min_cut: the global relabel did not settle");
      WSIS_HIP_CHECK(hipMemsetAsync(counters, 0, sizeof(host), st));
      for (int i = 0; i < CP_RELAX_BATCH; ++i) {
        hipLaunchKernelGGL(cp_relax_kernel, grid, block, 0, st, ex, V, A, d_arc_off, d_arc_head, res, h, counters + i);
        WSIS_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL(cp_active_kernel, grid, block, 0, st, ex, h, V, counters + CP_RELAX_BATCH);
      WSIS_LAUNCH_CHECK();
      WSIS_HIP_CHECK(hipMemcpyAsync(host, counters, sizeof(host), hipMemcpyDeviceToHost, st));
      WSIS_HIP_CHECK(hipStreamSynchronize(st));
    }
    const int32_t active = host[CP_RELAX_BATCH];
    if (active == 0) break;                     // no excess can reach the sink: the preflow is maximal
    if (rounds >= max_rounds) {
      *h_rounds = rounds;
      return fail(WSIS_ERR_OVERFLOW, "wsis_cp_min_cut: %d rounds did not finish the flow (%d active nodes left)", rounds,
                  active);
    }
    for (int i = 0; i < CP_PUSH_LAUNCHES; ++i) {
      hipLaunchKernelGGL(cp_push_kernel, grid, block, 0, st, ex, V, d_arc_off, d_arc_head, d_arc_rev, A, res, h);
      WSIS_LAUNCH_CHECK();
    }
    ++rounds;
  }
  *h_rounds = rounds;
  WSIS_HIP_CHECK(hipMemsetAsync(d_cut, 0, 8, st));
  hipLaunchKernelGGL(cp_cut_kernel, grid, block, 0, st, h, V, d_src_cap, d_snk_cap, d_arc_off, d_arc_head, d_arc_cap, d_sink_side,
                     reinterpret_cast<unsigned long long*>(d_cut));
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_cp_activate_workspace_bytes(int64_t V) {
  if (V < 1 || V >= ((int64_t)1 << 30)) return -1;
  return (int64_t)(2 * cp_align((size_t)V * 4) + 256);
}

int wsis_cp_activate(const int32_t* d_source, const int32_t* d_target, int64_t E, const uint8_t* d_label,
                     const int32_t* d_comp, const int32_t* d_comp_off, const int32_t* d_comp_nodes, int64_t C, int64_t V,
                     uint8_t* d_sat, uint8_t* d_active, int32_t* d_comp_new, uint8_t* d_sat_new, int32_t* d_count,
                     int32_t* h_rounds, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(V >= 1 && C >= 1 && C <= V && V < ((int64_t)1 << 30), "1 <= C <= V < 2^30");
  WSIS_REQUIRE(E >= 0 && E < ((int64_t)1 << 29), "0 <= E < 2^29");
  WSIS_REQUIRE(d_label && d_comp && d_comp_off && d_comp_nodes && d_sat && d_comp_new && d_sat_new && d_count && h_rounds && d_ws,
               "null pointer");
  WSIS_REQUIRE(E == 0 || (d_source && d_target && d_active), "null pointer");
  WSIS_REQUIRE(ws_bytes >= wsis_cp_activate_workspace_bytes(V), "workspace too small");
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(d_ws);
  int32_t* parent = reinterpret_cast<int32_t*>(ws);
  int32_t* rank = reinterpret_cast<int32_t*>(ws + cp_align((size_t)V * 4));
  int32_t* changed = reinterpret_cast<int32_t*>(ws + 2 * cp_align((size_t)V * 4));
  const dim3 gv(grid_for(V, CP_BLOCK)), ge(grid_for(E, CP_BLOCK)), block(CP_BLOCK);
  hipLaunchKernelGGL(cp_saturate_kernel, dim3(comp_grid(C)), block, 0, st, d_comp_off, d_comp_nodes, C, d_label, d_sat);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_iota_kernel, gv, block, 0, st, parent, V);
  WSIS_LAUNCH_CHECK();
  int32_t rounds = 0;
  if (E > 0) {
    hipLaunchKernelGGL(cp_activate_kernel, ge, block, 0, st, d_source, d_target, E, d_label, d_active);
    WSIS_LAUNCH_CHECK();
    // every round lowers a parent or ends the loop: it ends; the bound is a guard, far above what hooking by roots needs
    for (int32_t host = 1; host; ++rounds) {
      if (rounds > 64 + V) return fail(WSIS_ERR_OVERFLOW, "wsis_cp_activate: the components did not settle");
      WSIS_HIP_CHECK(hipMemsetAsync(changed, 0, 4, st));
      hipLaunchKernelGGL(cp_hook_kernel, ge, block, 0, st, d_source, d_target, E, d_active, parent, changed);
      WSIS_LAUNCH_CHECK();
      hipLaunchKernelGGL(cp_compress_kernel, gv, block, 0, st, parent, V);
      WSIS_LAUNCH_CHECK();
      WSIS_HIP_CHECK(hipMemcpyAsync(&host, changed, 4, hipMemcpyDeviceToHost, st));
      WSIS_HIP_CHECK(hipStreamSynchronize(st));
    }
  }
  *h_rounds = rounds;
  hipLaunchKernelGGL(cp_rootflag_kernel, gv, block, 0, st, parent, V, rank);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_scan_kernel, dim3(1), dim3(CP_SCAN_BLOCK), 0, st, rank, V, d_count);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_newcomp_kernel, gv, block, 0, st, parent, rank, V, d_comp, d_sat, C, d_comp_new, d_sat_new);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_cp_values(const float* d_features, int32_t D, const int32_t* d_comp_off, const int32_t* d_comp_nodes, int64_t C,
                   double* d_mean, double* d_weight, void* stream) {
  WSIS_REQUIRE(C >= 1 && C < ((int64_t)1 << 30), "1 <= C < 2^30");
  WSIS_REQUIRE(D >= 1 && D <= CP_DMAX, "1 <= D <= 8");
  WSIS_REQUIRE(d_features && d_comp_off && d_comp_nodes && d_mean && d_weight, "null pointer");
  hipLaunchKernelGGL(cp_values_kernel, dim3(comp_grid(C)), dim3(CP_BLOCK), 0, as_stream(stream), d_features, D, d_comp_off,
                     d_comp_nodes, C, d_mean, d_weight);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_cp_border_keys(const int32_t* d_source, const int32_t* d_target, const int32_t* d_comp, int64_t E, int64_t C,
                        int64_t* d_keys, void* stream) {
  WSIS_REQUIRE(E >= 0 && E < ((int64_t)1 << 29) && C >= 1 && C < ((int64_t)1 << 30), "0 <= E < 2^29, 1 <= C < 2^30");
  if (E == 0) return WSIS_OK;
  WSIS_REQUIRE(d_source && d_target && d_comp && d_keys, "null pointer");
  hipLaunchKernelGGL(cp_border_keys_kernel, dim3(grid_for(E, CP_BLOCK)), dim3(CP_BLOCK), 0, as_stream(stream), d_source, d_target,
                     d_comp, E, C, d_keys);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_cp_borders(const int64_t* d_ukeys, const int64_t* d_border_off, const int64_t* d_order, const float* d_edge_weight,
                    int64_t E, const double* d_mean, const double* d_weight, int32_t D, double lam, int64_t B, int64_t C,
                    int32_t* d_ba, int32_t* d_bb, double* d_bw, double* d_gain, void* stream) {
  WSIS_REQUIRE(B >= 0 && B <= E && C >= 1 && C < ((int64_t)1 << 30), "0 <= B <= E, 1 <= C < 2^30");
  WSIS_REQUIRE(D >= 1 && D <= CP_DMAX, "1 <= D <= 8");
  if (B == 0) return WSIS_OK;
  WSIS_REQUIRE(d_ukeys && d_border_off && d_order && d_edge_weight && d_mean && d_weight && d_ba && d_bb && d_bw && d_gain,
               "null pointer");
  hipLaunchKernelGGL(cp_borders_kernel, dim3(grid_for(B, CP_BLOCK)), dim3(CP_BLOCK), 0, as_stream(stream), d_ukeys, d_border_off,
                     d_order, d_edge_weight, E, d_mean, d_weight, D, lam, B, C, d_ba, d_bb, d_bw, d_gain);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_cp_merge_workspace_bytes(int64_t C) {
  if (C < 1 || C >= ((int64_t)1 << 30)) return -1;
  return (int64_t)(cp_align((size_t)C * 8) + cp_align((size_t)C * 4) + 2 * cp_align((size_t)C) + 256);
}

int wsis_cp_merge(const int32_t* d_ba, const int32_t* d_bb, const double* d_gain, int64_t B, int64_t C, uint8_t* d_taken,
                  int32_t* d_map, int32_t* h_rounds, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(C >= 1 && C < ((int64_t)1 << 30) && B >= 0 && B < ((int64_t)1 << 30), "1 <= C < 2^30, 0 <= B < 2^30");
  WSIS_REQUIRE(d_map && h_rounds && d_ws, "null pointer");
  WSIS_REQUIRE(B == 0 || (d_ba && d_bb && d_gain && d_taken), "null pointer");
  WSIS_REQUIRE(ws_bytes >= wsis_cp_merge_workspace_bytes(C), "workspace too small");
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(d_ws);
  unsigned long long* best_gain = reinterpret_cast<unsigned long long*>(ws);
  int32_t* best_idx = reinterpret_cast<int32_t*>(ws + cp_align((size_t)C * 8));
  uint8_t* matched = reinterpret_cast<uint8_t*>(ws + cp_align((size_t)C * 8) + cp_align((size_t)C * 4));
  int32_t* took = reinterpret_cast<int32_t*>(matched + 2 * cp_align((size_t)C));
  const dim3 gc(grid_for(C, CP_BLOCK)), gb(grid_for(B, CP_BLOCK)), block(CP_BLOCK);
  hipLaunchKernelGGL(cp_iota_kernel, gc, block, 0, st, d_map, C);
  WSIS_LAUNCH_CHECK();
  int32_t rounds = 0;
  if (B > 0) {
    WSIS_HIP_CHECK(hipMemsetAsync(matched, 0, (size_t)C, st));
    WSIS_HIP_CHECK(hipMemsetAsync(d_taken, 0, (size_t)B, st));
    // the best live border overall dominates at both its ends: every round but the last takes one, B + 1 at the most
    for (int32_t host = 1; host; ++rounds) {
      if (rounds > B + 1) return fail(WSIS_ERR_OVERFLOW, "wsis_cp_merge: the matching did not settle");
      WSIS_HIP_CHECK(hipMemsetAsync(took, 0, 4, st));
      hipLaunchKernelGGL(cp_merge_reset_kernel, gc, block, 0, st, best_gain, best_idx, C);
      WSIS_LAUNCH_CHECK();
      hipLaunchKernelGGL(cp_merge_gain_kernel, gb, block, 0, st, d_ba, d_bb, d_gain, matched, B, best_gain);
      WSIS_LAUNCH_CHECK();
      hipLaunchKernelGGL(cp_merge_idx_kernel, gb, block, 0, st, d_ba, d_bb, d_gain, matched, B, best_gain, best_idx);
      WSIS_LAUNCH_CHECK();
      hipLaunchKernelGGL(cp_merge_take_kernel, gb, block, 0, st, d_ba, d_bb, d_gain, B, best_idx, matched, d_taken, d_map, took);
      WSIS_LAUNCH_CHECK();
      WSIS_HIP_CHECK(hipMemcpyAsync(&host, took, 4, hipMemcpyDeviceToHost, st));
      WSIS_HIP_CHECK(hipStreamSynchronize(st));
    }
  }
  *h_rounds = rounds;
  return WSIS_OK;
}

int64_t wsis_cp_relabel_workspace_bytes(int64_t C) {
  if (C < 1 || C >= ((int64_t)1 << 30)) return -1;
  return (int64_t)(cp_align((size_t)C * 4) + cp_align((size_t)C));
}

int wsis_cp_relabel(const int32_t* d_map, int64_t C, const int32_t* d_source, const int32_t* d_target, int64_t E,
                    const int32_t* d_comp, int64_t V, const uint8_t* d_sat, uint8_t* d_active, int32_t* d_comp_new,
                    uint8_t* d_sat_new, int32_t* d_count, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(V >= 1 && C >= 1 && C <= V && V < ((int64_t)1 << 30), "1 <= C <= V < 2^30");
  WSIS_REQUIRE(E >= 0 && E < ((int64_t)1 << 29), "0 <= E < 2^29");
  WSIS_REQUIRE(d_map && d_comp && d_sat && d_comp_new && d_sat_new && d_count && d_ws, "null pointer");
  WSIS_REQUIRE(E == 0 || (d_source && d_target && d_active), "null pointer");
  WSIS_REQUIRE(ws_bytes >= wsis_cp_relabel_workspace_bytes(C), "workspace too small");
  hipStream_t st = as_stream(stream);
  int32_t* newid = static_cast<int32_t*>(d_ws);
  uint8_t* merged = reinterpret_cast<uint8_t*>(static_cast<char*>(d_ws) + cp_align((size_t)C * 4));
  WSIS_HIP_CHECK(hipMemsetAsync(merged, 0, (size_t)C, st));
  hipLaunchKernelGGL(cp_keepflag_kernel, dim3(grid_for(C, CP_BLOCK)), dim3(CP_BLOCK), 0, st, d_map, C, newid, merged);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_scan_kernel, dim3(1), dim3(CP_SCAN_BLOCK), 0, st, newid, C, d_count);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_relabel_kernel, dim3(grid_for(E > V ? E : V, CP_BLOCK)), dim3(CP_BLOCK), 0, st, d_map, newid, merged, C,
                     d_source, d_target, E, d_comp, V, d_sat, d_active, d_comp_new, d_sat_new);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_cp_energy_workspace_bytes(void) { return (int64_t)cp_align((size_t)CP_ENERGY_GRID * 3 * 8); }

int wsis_cp_energy(const float* d_features, int32_t D, const int32_t* d_comp, const double* d_mean, int64_t V, int64_t C,
                   const int32_t* d_source, const int32_t* d_target, const float* d_edge_weight, int64_t E, double lam,
                   const uint8_t* d_sat, double* d_out3, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(V >= 1 && C >= 1 && C <= V && V < ((int64_t)1 << 30), "1 <= C <= V < 2^30");
  WSIS_REQUIRE(E >= 0 && E < ((int64_t)1 << 29), "0 <= E < 2^29");
  WSIS_REQUIRE(D >= 1 && D <= CP_DMAX, "1 <= D <= 8");
  WSIS_REQUIRE(d_features && d_comp && d_mean && d_sat && d_out3 && d_ws, "null pointer");
  WSIS_REQUIRE(E == 0 || (d_source && d_target && d_edge_weight), "null pointer");
  WSIS_REQUIRE(ws_bytes >= wsis_cp_energy_workspace_bytes(), "workspace too small");
  hipStream_t st = as_stream(stream);
  double* part = static_cast<double*>(d_ws);
  hipLaunchKernelGGL(cp_energy_part_kernel, dim3(CP_ENERGY_GRID), dim3(CP_BLOCK), 0, st, d_features, D, d_comp, d_mean, V, C,
                     d_source, d_target, d_edge_weight, E, d_sat, part);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_energy_finish_kernel, dim3(1), dim3(1), 0, st, part, CP_ENERGY_GRID, lam, d_out3);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
