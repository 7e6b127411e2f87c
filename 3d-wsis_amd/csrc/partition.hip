// The S3DIS partition front end (data/S3DIS/partition of the reference), the array stages before the l0 cut-pursuit
// solver of generate_SPG_superpoint (partition_S3DIS.py:81-115):
//
//   libply_c.prune, the voxel of every point       ply_c/ply_c.cpp:311-337            wsis_pt_bins
//   libply_c.prune, the voxel averages             ply_c/ply_c.cpp:255-290, 368-390   wsis_pt_prune_accumulate
//   compute_graph_nn_2 (sklearn kd-tree)           graphs.py:26-83                    wsis_pt_knn
//   libply_c.compute_geof (Eigen)                  ply_c/ply_c.cpp:396-474            wsis_pt_geof
//   features and edge weights                      partition_S3DIS.py:105-108         wsis_pt_edge_features
//
// The voxel ids between the first two are wsis_voxelize_idx_map (first-occurrence ids = the insertion index of the
// reference's std::map) and wsis_segment_csr (a voxel's points in ascending point index).
//
// Reproducibility: no floating-point atomic (the extrema go through integer atomics on an order-preserving encoding:
// min and max do not depend on the order of arrival).  A voxel's sums are one sequential chain in point order, a
// neighbour list is the k smallest (d2, id) pairs -- a total order, independent of how candidates arrive -- and the
// mean distance is summed in sequential chains in index order.  Products and sums stay uncontracted (-ffp-contract=off).  Two calls give
// the same bytes.  Every index read from a table is clamped to its table before use.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

using namespace wsis;

namespace {

constexpr int PT_BLOCK = 256;
constexpr int PT_WAVES = PT_BLOCK / 64;
constexpr int PT_K_MAX = 64;                     // one (d2, id) pair of the running list per lane
constexpr int PT_RING_MAX = 3;                   // rings of cells visited before a query scans every point instead
constexpr int PT_SWEEPS = 12;                    // cyclic Jacobi on a 3x3 converges quadratically: 5-6 sweeps in practice
constexpr int PT_CELL_BITS = 21;                 // cells per axis < 2^21: three indices in one 64-bit key
// points per cell the automatic cell edge aims at for a cloud that FILLS its box / face / edge.  Scanned rooms are
// surfaces in a box: the box estimate wins and a cell on a surface then holds several times this figure (a few tens)
constexpr double PT_OCCUPANCY = 8.0;
constexpr int PT_SUM_CHUNK = 256;                // consecutive distances one thread adds into one chunk sum of the mean

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ __forceinline__ double pt_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// order-preserving map of fp32 onto uint32: integer atomicMin / atomicMax then give the floating-point extrema
__device__ __forceinline__ uint32_t pt_encode(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pt_decode(uint32_t e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

// enc[0..3) = encoded minima (start 0xffffffff), enc[3..6) = encoded maxima (start 0), enc[6] = 1 if a coordinate is
// not finite.  NaN takes no part in the extrema.
__global__ __launch_bounds__(PT_BLOCK) void pt_extrema_kernel(const float* __restrict__ xyz, int64_t N,
                                                              uint32_t* __restrict__ enc) {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  int bad = 0;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = xyz[3 * p + a];
      if (!(fabsf(x) <= 3.402823466e38f)) bad = 1;
      if (x == x) {
        const uint32_t e = pt_encode(x);
        lo[a] = min(lo[a], e);
        hi[a] = max(hi[a], e);
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], m));
      hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], m));
    }
    bad |= __shfl_xor(bad, m);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(enc + a, lo[a]);
      atomicMax(enc + 3 + a, hi[a]);
    }
    if (bad) atomicOr(enc + 6, 1u);
  }
}

__global__ void pt_extrema_init_kernel(uint32_t* __restrict__ enc) {
  if (threadIdx.x < 3) enc[threadIdx.x] = 0xffffffffu;
  else if (threadIdx.x < 7) enc[threadIdx.x] = 0u;
}

// ---- the voxel of every point: (0, bx, by, bz), b = floorf((x - x_min) / voxel) in fp32, not clamped to n_bin
__global__ __launch_bounds__(PT_BLOCK) void pt_bins_kernel(const float* __restrict__ xyz, int64_t N, float voxel,
                                                           const uint32_t* __restrict__ enc, int64_t* __restrict__ coords,
                                                           float* __restrict__ min3, int32_t* __restrict__ nonfinite) {
  const float mn[3] = {pt_decode(enc[0]), pt_decode(enc[1]), pt_decode(enc[2])};
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    min3[0] = mn[0];
    min3[1] = mn[1];
    min3[2] = mn[2];
    *nonfinite = (int32_t)enc[6];
  }
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
    coords[4 * p] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float t = floorf(__fdiv_rn(xyz[3 * p + a] - mn[a], voxel));
      // a quotient that is not finite has no bin: such input is refused by the caller, the value only has to be defined
      coords[4 * p + 1 + a] = (fabsf(t) <= 9.0e18f) ? (int64_t)t : 0;
    }
  }
}

// ---- the averages of every voxel: one thread walks one row of the CSR in point order
__global__ __launch_bounds__(PT_BLOCK) void pt_prune_kernel(const float* __restrict__ xyz, const uint8_t* __restrict__ rgb,
                                                            const int32_t* __restrict__ labels, int32_t n_labels,
                                                            const int32_t* __restrict__ perm,
                                                            const int32_t* __restrict__ offsets, int64_t N, int64_t V,
                                                            float* __restrict__ out_xyz, uint8_t* __restrict__ out_rgb,
                                                            uint32_t* __restrict__ hist, int32_t* __restrict__ count) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v >= V) return;
  int64_t b = offsets[v], e = offsets[v + 1];
  b = b < 0 ? 0 : (b > N ? N : b);
  e = e < b ? b : (e > N ? N : e);
  const int width = n_labels + 1;
  uint32_t* __restrict__ h = labels ? hist + v * width : nullptr;
  if (h)
    for (int c = 0; c < width; ++c) h[c] = 0u;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  uint32_t sr = 0u, sg = 0u, sb = 0u;
  for (int64_t j = b; j < e; ++j) {
    int64_t p = perm[j];
    p = p < 0 ? 0 : (p >= N ? N - 1 : p);
    sx = sx + xyz[3 * p];
    sy = sy + xyz[3 * p + 1];
    sz = sz + xyz[3 * p + 2];
    sr += rgb[3 * p];
    sg += rgb[3 * p + 1];
    sb += rgb[3 * p + 2];
    if (h) {
      const int32_t l = labels[p];
      if (l >= 0 && l < width) h[l] += 1u;        // a label above n_labels is refused before the launch
    }
  }
  const float n = (float)(e - b);
  out_xyz[3 * v] = __fdiv_rn(sx, n);
  out_xyz[3 * v + 1] = __fdiv_rn(sy, n);
  out_xyz[3 * v + 2] = __fdiv_rn(sz, n);
  // (uint8_t)(float): truncation; an empty row (0 / 0) cannot occur for ids that come from the map, and writes 0
  const float r = __fdiv_rn((float)sr, n), g = __fdiv_rn((float)sg, n), bl = __fdiv_rn((float)sb, n);
  out_rgb[3 * v] = e > b ? (uint8_t)(int)r : (uint8_t)0;
  out_rgb[3 * v + 1] = e > b ? (uint8_t)(int)g : (uint8_t)0;
  out_rgb[3 * v + 2] = e > b ? (uint8_t)(int)bl : (uint8_t)0;
  count[v] = (int32_t)(e - b);
}

// ---- k nearest neighbours over a uniform grid of cells found through the sorted cell keys ----------------------------
struct PtGrid {
  double mn[3];
  double cell;
  int32_t dim[3];
  int32_t pad;
};

// the grid of a cloud: the cell edge the caller gave, or one that aims at PT_OCCUPANCY points per cell for a cloud that
// fills its bounding box, its largest face or its longest edge (whichever asks for the largest cell); never so small
// that an axis would have 2^20 cells or more
__global__ void pt_grid_kernel(const uint32_t* __restrict__ enc, int64_t V, double cell_in, PtGrid* __restrict__ grid) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double ext[3];
  for (int a = 0; a < 3; ++a) {
    const double lo = (double)pt_decode(enc[a]), hi = (double)pt_decode(enc[3 + a]);
    grid->mn[a] = lo;
    ext[a] = hi - lo;
    if (!(ext[a] >= 0.0) || !(ext[a] <= 1e300)) ext[a] = 0.0;      // no finite point on this axis
    if (!(fabs(lo) <= 1e300)) grid->mn[a] = 0.0;
  }
  double cell = cell_in;
  if (!(cell > 0.0) || !(cell <= 1e300)) {
    const double w = PT_OCCUPANCY / (double)V;
    const double face = fmax(ext[0] * ext[1], fmax(ext[0] * ext[2], ext[1] * ext[2]));
    const double edge = fmax(ext[0], fmax(ext[1], ext[2]));
    cell = fmax(cbrt(ext[0] * ext[1] * ext[2] * w), fmax(sqrt(face * w), edge * w));
    if (!(cell > 0.0)) cell = 1.0;               // every point at one place
  }
  const double longest = fmax(ext[0], fmax(ext[1], ext[2]));
  cell = fmax(cell, longest / 1048576.0);
  grid->cell = cell;
  for (int a = 0; a < 3; ++a) {
    double d = floor(ext[a] / cell) + 1.0;
    if (!(d >= 1.0)) d = 1.0;
    if (d > 2097151.0) d = 2097151.0;
    grid->dim[a] = (int32_t)d;
  }
  grid->pad = 0;
}

__device__ __forceinline__ int pt_cell_of(double x, double mn, double cell, int dim) {
  const double t = floor((x - mn) / cell);
  if (!(t >= 0.0)) return 0;                     // also NaN
  return t >= (double)dim ? dim - 1 : (int)t;
}
__device__ __forceinline__ uint64_t pt_key(int cx, int cy, int cz) {
  return ((uint64_t)cz << (2 * PT_CELL_BITS)) | ((uint64_t)cy << PT_CELL_BITS) | (uint64_t)cx;
}

__global__ __launch_bounds__(PT_BLOCK) void pt_keys_kernel(const float* __restrict__ xyz, int64_t V,
                                                           const PtGrid* __restrict__ grid, uint64_t* __restrict__ keys,
                                                           int32_t* __restrict__ iota) {
  const PtGrid g = *grid;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < V; p += (int64_t)gridDim.x * blockDim.x) {
    const int cx = pt_cell_of((double)xyz[3 * p], g.mn[0], g.cell, g.dim[0]);
    const int cy = pt_cell_of((double)xyz[3 * p + 1], g.mn[1], g.cell, g.dim[1]);
    const int cz = pt_cell_of((double)xyz[3 * p + 2], g.mn[2], g.cell, g.dim[2]);
    keys[p] = pt_key(cx, cy, cz);
    iota[p] = (int32_t)p;
  }
}

// the points in cell order: the candidate loads of a query are then runs of consecutive 12-byte rows
__global__ __launch_bounds__(PT_BLOCK) void pt_gather_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ ids,
                                                             int64_t V, float* __restrict__ sorted_xyz) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < V; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t p = ids[j];
    p = p < 0 ? 0 : (p >= V ? V - 1 : p);
    sorted_xyz[3 * j] = xyz[3 * p];
    sorted_xyz[3 * j + 1] = xyz[3 * p + 1];
    sorted_xyz[3 * j + 2] = xyz[3 * p + 2];
  }
}

// first position of the sorted keys that is not below `key`
__device__ __forceinline__ int pt_lower_bound(const uint64_t* __restrict__ keys, int n, uint64_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool pt_less(double d0, int i0, double d1, int i1) { return d0 < d1 || (d0 == d1 && i0 < i1); }

// one compare-exchange step of a bitonic network between lane and lane ^ m: the lane keeps the smaller pair if keep_min
__device__ __forceinline__ void pt_cmpx(double& d, int& i, int m, bool keep_min) {
  const double od = __shfl_xor(d, m);
  const int oi = __shfl_xor(i, m);
  const bool take = keep_min ? pt_less(od, oi, d, i) : pt_less(d, i, od, oi);
  if (take) {
    d = od;
    i = oi;
  }
}

// the running list (ascending over the lanes) takes a batch of 64 candidates: the batch is sorted ascending, the lower
// half of the union is min(list[l], batch[63 - l]) -- a bitonic sequence --, and six more steps sort it
__device__ __forceinline__ void pt_merge(double& bd, int& bi, double d, int i, int lane) {
#pragma unroll
  for (int k2 = 2; k2 <= 64; k2 <<= 1) {
#pragma unroll
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      const bool up = (lane & k2) == 0;            // k2 == 64: every lane
      const bool lower = (lane & j) == 0;
      pt_cmpx(d, i, j, lower == up);
    }
  }
  const double rd = __shfl(d, 63 - lane);
  const int ri = __shfl(i, 63 - lane);
  if (pt_less(rd, ri, bd, bi)) {
    bd = rd;
    bi = ri;
  }
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) pt_cmpx(bd, bi, j, (lane & j) == 0);
}

// one batch: lane l evaluates the point at position `pos` of the cell order (valid lanes only)
__device__ __forceinline__ void pt_take(const float* __restrict__ sxyz, const int32_t* __restrict__ ids, int iV, int pos,
                                        bool valid, int qid, double qx, double qy, double qz, int k, int lane, double& bd,
                                        int& bi) {
  double d = pt_inf();
  int id = 0x7fffffff;
  if (valid) {
    pos = pos < 0 ? 0 : (pos >= iV ? iV - 1 : pos);
    int c = ids[pos];
    c = c < 0 ? 0 : (c >= iV ? iV - 1 : c);
    if (c != qid) {                                // self is excluded by id
      const double dx = (double)sxyz[3 * (int64_t)pos] - qx, dy = (double)sxyz[3 * (int64_t)pos + 1] - qy,
                   dz = (double)sxyz[3 * (int64_t)pos + 2] - qz;
      d = (dx * dx + dy * dy) + dz * dz;
      id = c;
    }
  }
  const double kd = __shfl(bd, k - 1);
  const int ki = __shfl(bi, k - 1);
  if (__ballot(pt_less(d, id, kd, ki)) != 0ull) pt_merge(bd, bi, d, id, lane);      // wave-uniform
}

// One wave per query, queries in cell order.  Ring r = the cells at Chebyshev distance r of the query's cell.  A ring is
// dealt to the lanes as spans of consecutive positions of the cell order: along x the keys of one (y, z) row are
// consecutive, so a whole row of the ring's two z / y faces is one span, and the two x faces give one cell per row.
__global__ __launch_bounds__(PT_BLOCK) void pt_knn_kernel(const float* __restrict__ sxyz, const uint64_t* __restrict__ keys,
                                                          const int32_t* __restrict__ ids, const PtGrid* __restrict__ grid,
                                                          int64_t V, int k, int32_t* __restrict__ nbr,
                                                          double* __restrict__ dist2, int32_t* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * PT_WAVES + (threadIdx.x >> 6);
  if (w >= V) return;                            // wave-uniform
  const int iV = (int)V;
  const PtGrid g = *grid;
  int qid = ids[w];
  qid = qid < 0 ? 0 : (qid >= iV ? iV - 1 : qid);
  const double q[3] = {(double)sxyz[3 * w], (double)sxyz[3 * w + 1], (double)sxyz[3 * w + 2]};
  const uint64_t qk = keys[w];
  const int cmask = (1 << PT_CELL_BITS) - 1;
  int c[3] = {(int)(qk & cmask), (int)((qk >> PT_CELL_BITS) & cmask), (int)((qk >> (2 * PT_CELL_BITS)) & cmask)};
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = c[a] >= g.dim[a] ? g.dim[a] - 1 : c[a];
  double bd = pt_inf();
  int bi = 0x7fffffff;
  int ncand = 0, fallback = 0;
  for (int r = 0;; ++r) {
    if (r > PT_RING_MAX) {                         // an isolated query: every point, once
      fallback = 1;
      bd = pt_inf();
      bi = 0x7fffffff;
      for (int j0 = 0; j0 < iV; j0 += 64) {
        const int j = j0 + lane;
        pt_take(sxyz, ids, iV, j, j < iV, qid, q[0], q[1], q[2], k, lane, bd, bi);
      }
      ncand += iV;
      break;
    }
    const int side = 2 * r + 1, nslots = 2 * side * side;
    for (int s0 = 0; s0 < nslots; s0 += 64) {
      const int s = s0 + lane;
      int start = 0, cnt = 0;
      if (s < nslots) {
        const int half = s & 1, yz = s >> 1;
        const int dy = yz % side - r, dz = yz / side - r;
        const int y = c[1] + dy, z = c[2] + dz;
        const bool face = (dy == r || dy == -r || dz == r || dz == -r);
        int x0, x1;
        if (face) {
          x0 = c[0] - r;
          x1 = half == 0 ? c[0] + r : x0 - 1;      // the row once
        } else {
          x0 = x1 = half == 0 ? c[0] - r : c[0] + r;
        }
        x0 = x0 < 0 ? 0 : x0;
        x1 = x1 >= g.dim[0] ? g.dim[0] - 1 : x1;
        if (y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2] && x0 <= x1) {
          start = pt_lower_bound(keys, iV, pt_key(x0, y, z));
          cnt = pt_lower_bound(keys, iV, pt_key(x1, y, z) + 1) - start;
          cnt = cnt < 0 ? 0 : cnt;
        }
      }
      int pre = cnt;                               // inclusive prefix over the lanes
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_up(pre, m);
        if (lane >= m) pre += o;
      }
      const int total = __shfl(pre, 63);
      pre -= cnt;                                  // exclusive
      for (int b = 0; b < total; b += 64) {        // wave-uniform
        const int j = b + lane;
        int t = 0;                                 // the last span that starts at or before j
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
          const int p = __shfl(pre, t + step);
          if (p <= j) t += step;
        }
        const int pos = __shfl(start, t) + (j - __shfl(pre, t));
        pt_take(sxyz, ids, iV, pos, j < total, qid, q[0], q[1], q[2], k, lane, bd, bi);
      }
      ncand += total;
    }
    // a point outside the searched block lies beyond one of its faces that has cells behind it
    double m = pt_inf();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (c[a] - r > 0) m = fmin(m, q[a] - (g.mn[a] + (double)(c[a] - r) * g.cell));
      if (c[a] + r < g.dim[a] - 1) m = fmin(m, (g.mn[a] + (double)(c[a] + r + 1) * g.cell) - q[a]);
    }
    if (m == pt_inf()) break;                      // the block covers the grid
    // the cell of a point is a rounded quotient and the face a rounded product: stay inside the face
    m -= 1e-7 * g.cell + 1e-14 * (fabs(q[0]) + fabs(q[1]) + fabs(q[2]));
    const double kd = __shfl(bd, k - 1);
    if (m > 0.0 && kd < m * m) break;
  }
  if (lane < k) {
    nbr[(int64_t)qid * k + lane] = bi;
    dist2[(int64_t)qid * k + lane] = bd;
  }
  if (stats && lane == 0) {
    stats[2 * (int64_t)qid] = ncand;
    stats[2 * (int64_t)qid + 1] = fallback;
  }
}

// ---- geometric features ----------------------------------------------------------------------------------------------
// one Jacobi rotation that annihilates a_pq (r: the third index; a_rp, a_rq the other two off-diagonal entries) and
// turns the columns p, q of the eigenvector matrix
__device__ __forceinline__ void pt_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double* vp,
                                          double* vq) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double a = vp[i], b = vq[i];
    vp[i] = c * a - s * b;
    vq[i] = s * a + c * b;
  }
}

// eigenvalues (descending) and unit eigenvectors vec[j][0..3) of the symmetric 3x3 (xx, yy, zz, xy, xz, yz)
__device__ __forceinline__ void pt_eig3(double xx, double yy, double zz, double xy, double xz, double yz, double* ev,
                                        double vec[3][3]) {
  double vx[3] = {1.0, 0.0, 0.0}, vy[3] = {0.0, 1.0, 0.0}, vz[3] = {0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < PT_SWEEPS; ++sweep) {
    const double off = fabs(xy) + fabs(xz) + fabs(yz);
    if (off == 0.0 || off <= 1e-300 + 1e-22 * (fabs(xx) + fabs(yy) + fabs(zz))) break;
    pt_rotate(xx, yy, xy, xz, yz, vx, vy);
    pt_rotate(xx, zz, xz, xy, yz, vx, vz);
    pt_rotate(yy, zz, yz, xy, xz, vy, vz);
  }
  double l[3] = {xx, yy, zz};
  int o[3] = {0, 1, 2};
  auto swap = [&](int a, int b) {
    if (l[a] < l[b]) {
      const double t = l[a];
      l[a] = l[b];
      l[b] = t;
      const int u = o[a];
      o[a] = o[b];
      o[b] = u;
    }
  };
  swap(0, 1);
  swap(1, 2);
  swap(0, 1);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    ev[j] = l[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) vec[j][i] = o[j] == 0 ? vx[i] : (o[j] == 1 ? vy[i] : vz[i]);
  }
}

__global__ __launch_bounds__(PT_BLOCK) void pt_geof_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ nbr,
                                                           int64_t V, int k, float* __restrict__ geof,
                                                           double* __restrict__ cov6, double* __restrict__ ev3) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int32_t* __restrict__ row = nbr + v * k;
  auto point = [&](int j, double* p) {             // j = 0: the point itself, then its neighbours in list order
    int64_t i = v;
    if (j > 0) {
      i = row[j - 1];
      i = i < 0 ? 0 : (i >= V ? V - 1 : i);
    }
    p[0] = (double)xyz[3 * i];
    p[1] = (double)xyz[3 * i + 1];
    p[2] = (double)xyz[3 * i + 2];
  };
  const double n = (double)(k + 1);
  double s[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j <= k; ++j) {
    double p[3];
    point(j, p);
    s[0] += p[0];
    s[1] += p[1];
    s[2] += p[2];
  }
  const double mx = s[0] / n, my = s[1] / n, mz = s[2] / n;
  double cxx = 0.0, cyy = 0.0, czz = 0.0, cxy = 0.0, cxz = 0.0, cyz = 0.0;
  for (int j = 0; j <= k; ++j) {
    double p[3];
    point(j, p);
    const double dx = p[0] - mx, dy = p[1] - my, dz = p[2] - mz;
    cxx += dx * dx;
    cyy += dy * dy;
    czz += dz * dz;
    cxy += dx * dy;
    cxz += dx * dz;
    cyz += dy * dz;
  }
  cxx /= n;
  cyy /= n;
  czz /= n;
  cxy /= n;
  cxz /= n;
  cyz /= n;
  double ev[3], vec[3][3];
  pt_eig3(cxx, cyy, czz, cxy, cxz, cyz, ev, vec);
  const double l0 = fmax(ev[0], 0.0), l1 = fmax(ev[1], 0.0), l2 = fmax(ev[2], 0.0);
  const double r0 = sqrt(l0), r1 = sqrt(l1), r2 = sqrt(l2);
  const double lin = (r0 - r1) / r0, plan = (r1 - r2) / r0, scat = r2 / r0;      // l0 == 0: NaN, as the reference's
  double u[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = (l0 * fabs(vec[0][i]) + l1 * fabs(vec[1][i])) + l2 * fabs(vec[2][i]);
  const double norm = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  const double vert = u[2] / norm;
  geof[4 * v] = (float)lin;
  geof[4 * v + 1] = (float)plan;
  geof[4 * v + 2] = (float)scat;
  geof[4 * v + 3] = (float)vert;
  if (cov6) {
    cov6[6 * v] = cxx;
    cov6[6 * v + 1] = cyy;
    cov6[6 * v + 2] = czz;
    cov6[6 * v + 3] = cxy;
    cov6[6 * v + 4] = cxz;
    cov6[6 * v + 5] = cyz;
  }
  if (ev3) {
    ev3[3 * v] = l0;
    ev3[3 * v + 1] = l1;
    ev3[3 * v + 2] = l2;
  }
}

// ---- feature matrix and edge weights ---------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_BLOCK) void pt_edge_dist_kernel(const int32_t* __restrict__ nbr,
                                                                const double* __restrict__ dist2, int64_t V, int k,
                                                                int k_adj, float* __restrict__ distances,
                                                                uint32_t* __restrict__ source, uint32_t* __restrict__ target) {
  const int64_t E = V * k_adj;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = e / k_adj;
    const int j = (int)(e - v * k_adj);
    int32_t t = nbr[v * k + j];
    t = t < 0 ? 0 : (t >= V ? (int32_t)(V - 1) : t);
    distances[e] = (float)sqrt(dist2[v * k + j]);
    source[e] = (uint32_t)v;
    target[e] = (uint32_t)t;
  }
}

// The mean of the distances: the fp64 sum in index order, as two levels of sequential chains.  One thread adds one
// chunk of PT_SUM_CHUNK consecutive distances in index order; one thread then adds the chunk sums in index order.  The
// result depends on PT_SUM_CHUNK alone, not on the shape of a launch.
__global__ __launch_bounds__(PT_BLOCK) void pt_edge_partial_kernel(const float* __restrict__ distances, int64_t E,
                                                                   int64_t n_partial, double* __restrict__ partial) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= n_partial) return;
  const int64_t e0 = c * PT_SUM_CHUNK, e1 = e0 + PT_SUM_CHUNK < E ? e0 + PT_SUM_CHUNK : E;
  double acc = 0.0;
  for (int64_t e = e0; e < e1; ++e) acc += (double)distances[e];
  partial[c] = acc;
}

__global__ void pt_edge_mean_kernel(const double* __restrict__ partial, int64_t n_partial, int64_t E,
                                    float* __restrict__ mean) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double acc = 0.0;
  for (int64_t i = 0; i < n_partial; ++i) acc += partial[i];
  *mean = (float)(acc / (double)E);
}

__global__ __launch_bounds__(PT_BLOCK) void pt_edge_weight_kernel(const float* __restrict__ distances, int64_t E,
                                                                  const float* __restrict__ mean, float lambda,
                                                                  float* __restrict__ weight) {
  const float m = *mean;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x)
    weight[e] = __fdiv_rn(1.f, lambda + __fdiv_rn(distances[e], m));
}

__global__ __launch_bounds__(PT_BLOCK) void pt_features_kernel(const float* __restrict__ geof, const uint8_t* __restrict__ rgb,
                                                               int64_t V, float* __restrict__ features) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    float* __restrict__ f = features + 7 * v;
    f[0] = geof[4 * v];
    f[1] = geof[4 * v + 1];
    f[2] = geof[4 * v + 2];
    f[3] = 2.f * geof[4 * v + 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) f[4 + c] = (float)((double)rgb[3 * v + c] / 255.0);
  }
}

int pt_extrema(const float* d_xyz, int64_t N, uint32_t* enc, hipStream_t st) {
  hipLaunchKernelGGL(pt_extrema_init_kernel, dim3(1), dim3(64), 0, st, enc);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pt_extrema_kernel, dim3(grid_for(N, PT_BLOCK)), dim3(PT_BLOCK), 0, st, d_xyz, N, enc);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

struct KnnLayout {
  size_t enc, grid, keys, keys_sorted, iota, ids, sxyz, temp, total;
};

int knn_temp_bytes(int64_t V, size_t* out) {
  uint64_t* kp = nullptr;
  int32_t* ip = nullptr;
  size_t bytes = 0;
  if (rocprim::radix_sort_pairs(nullptr, bytes, kp, kp, ip, ip, (size_t)V, 0, 3 * PT_CELL_BITS, (hipStream_t)0) !=
      hipSuccess)
    return -1;
  *out = bytes;
  return 0;
}

KnnLayout knn_layout(int64_t V, size_t temp_bytes) {
  KnnLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += align256(bytes);
    return o;
  };
  L.enc = take(8 * sizeof(uint32_t));
  L.grid = take(sizeof(PtGrid));
  L.keys = take((size_t)V * 8);
  L.keys_sorted = take((size_t)V * 8);
  L.iota = take((size_t)V * 4);
  L.ids = take((size_t)V * 4);
  L.sxyz = take((size_t)V * 12);
  L.temp = take(temp_bytes);
  L.total = off + 256;
  return L;
}

}  // namespace

extern "C" {

int64_t wsis_pt_bins_workspace_bytes(int64_t N) { return N < 0 ? -1 : 256; }

int wsis_pt_bins(const float* d_xyz, int64_t N, float voxel, int64_t* d_coords, float* d_min3, int32_t* d_nonfinite,
                 void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(N >= 1, "no points");
  WSIS_REQUIRE(N < ((int64_t)1 << 30), "N too large for int32 maps");
  WSIS_REQUIRE(voxel > 0.f && voxel <= 3.402823466e38f, "voxel width must be positive and finite");
  WSIS_REQUIRE(d_xyz && d_coords && d_min3 && d_nonfinite && d_ws, "null pointer");
  WSIS_REQUIRE(ws_bytes >= 256, "workspace too small");
  hipStream_t st = as_stream(stream);
  uint32_t* enc = static_cast<uint32_t*>(d_ws);
  if (int rc = pt_extrema(d_xyz, N, enc, st)) return rc;
  hipLaunchKernelGGL(pt_bins_kernel, dim3(grid_for(N, PT_BLOCK)), dim3(PT_BLOCK), 0, st, d_xyz, N, voxel, enc, d_coords,
                     d_min3, d_nonfinite);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_pt_prune_accumulate(const float* d_xyz, const uint8_t* d_rgb, const int32_t* d_labels, int32_t n_labels,
                             const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t V, float* d_out_xyz,
                             uint8_t* d_out_rgb, uint32_t* d_label_hist, int32_t* d_count, void* stream) {
  WSIS_REQUIRE(N >= 1 && V >= 1 && V <= N, "1 <= V <= N");
  WSIS_REQUIRE(N < ((int64_t)1 << 30), "N too large for the int32 CSR");
  WSIS_REQUIRE(n_labels >= 0 && n_labels <= 65535, "0 <= n_labels <= 65535");
  WSIS_REQUIRE(d_xyz && d_rgb && d_perm && d_offsets && d_out_xyz && d_out_rgb && d_count, "null pointer");
  WSIS_REQUIRE(!d_labels || d_label_hist, "labels without a histogram");
  const int64_t g = ceil_div(V, PT_BLOCK);
  hipLaunchKernelGGL(pt_prune_kernel, dim3((unsigned)g), dim3(PT_BLOCK), 0, as_stream(stream), d_xyz, d_rgb, d_labels,
                     n_labels, d_perm, d_offsets, N, V, d_out_xyz, d_out_rgb, d_label_hist, d_count);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_pt_knn_workspace_bytes(int64_t V) {
  if (V < 1 || V >= ((int64_t)1 << 30)) return -1;
  size_t temp = 0;
  if (knn_temp_bytes(V, &temp) != 0) return -1;
  return (int64_t)knn_layout(V, temp).total;
}

int wsis_pt_knn(const float* d_xyz, int64_t V, int32_t k, double cell, int32_t* d_nbr, double* d_dist2, int32_t* d_stats,
                void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(k >= 1 && k <= PT_K_MAX, "1 <= k <= 64");
  WSIS_REQUIRE(V >= (int64_t)k + 1, "fewer than k + 1 points");
  WSIS_REQUIRE(V < ((int64_t)1 << 30), "V too large for int32 indices");
  WSIS_REQUIRE(d_xyz && d_nbr && d_dist2 && d_ws, "null pointer");
  size_t temp_bytes = 0;
  WSIS_REQUIRE(knn_temp_bytes(V, &temp_bytes) == 0, "rocprim size query failed");
  const KnnLayout L = knn_layout(V, temp_bytes);
  WSIS_REQUIRE((int64_t)L.total <= ws_bytes, "workspace too small");
  char* ws = static_cast<char*>(d_ws);
  uint32_t* enc = reinterpret_cast<uint32_t*>(ws + L.enc);
  PtGrid* grid = reinterpret_cast<PtGrid*>(ws + L.grid);
  uint64_t* keys = reinterpret_cast<uint64_t*>(ws + L.keys);
  uint64_t* keys_sorted = reinterpret_cast<uint64_t*>(ws + L.keys_sorted);
  int32_t* iota = reinterpret_cast<int32_t*>(ws + L.iota);
  int32_t* ids = reinterpret_cast<int32_t*>(ws + L.ids);
  float* sxyz = reinterpret_cast<float*>(ws + L.sxyz);
  hipStream_t st = as_stream(stream);
  if (int rc = pt_extrema(d_xyz, V, enc, st)) return rc;
  hipLaunchKernelGGL(pt_grid_kernel, dim3(1), dim3(64), 0, st, enc, V, cell, grid);
  WSIS_LAUNCH_CHECK();
  const int g = grid_for(V, PT_BLOCK);
  hipLaunchKernelGGL(pt_keys_kernel, dim3(g), dim3(PT_BLOCK), 0, st, d_xyz, V, grid, keys, iota);
  WSIS_LAUNCH_CHECK();
  size_t tb = temp_bytes;
  WSIS_HIP_CHECK(rocprim::radix_sort_pairs(ws + L.temp, tb, keys, keys_sorted, iota, ids, (size_t)V, 0, 3 * PT_CELL_BITS,
                                           st));
  hipLaunchKernelGGL(pt_gather_kernel, dim3(g), dim3(PT_BLOCK), 0, st, d_xyz, ids, V, sxyz);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pt_knn_kernel, dim3((unsigned)ceil_div(V, PT_WAVES)), dim3(PT_BLOCK), 0, st, sxyz, keys_sorted, ids,
                     grid, V, (int)k, d_nbr, d_dist2, d_stats);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_pt_geof(const float* d_xyz, const int32_t* d_nbr, int64_t V, int32_t k, float* d_geof, double* d_cov6,
                 double* d_ev3, void* stream) {
  WSIS_REQUIRE(k >= 1 && k <= PT_K_MAX, "1 <= k <= 64");
  WSIS_REQUIRE(V >= 1 && V < ((int64_t)1 << 30), "V outside 1 .. 2^30 - 1");
  WSIS_REQUIRE(d_xyz && d_nbr && d_geof, "null pointer");
  hipLaunchKernelGGL(pt_geof_kernel, dim3((unsigned)ceil_div(V, PT_BLOCK)), dim3(PT_BLOCK), 0, as_stream(stream), d_xyz,
                     d_nbr, V, (int)k, d_geof, d_cov6, d_ev3);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int64_t wsis_pt_edge_features_workspace_bytes(int64_t V, int32_t k_adj) {
  if (V < 1 || k_adj < 1 || k_adj > PT_K_MAX) return -1;
  return (int64_t)align256((size_t)ceil_div(V * k_adj, PT_SUM_CHUNK) * sizeof(double)) + 256;
}

int wsis_pt_edge_features(const float* d_geof, const uint8_t* d_rgb, const int32_t* d_nbr, const double* d_dist2, int64_t V,
                          int32_t k, int32_t k_adj, float lambda, float* d_features, uint32_t* d_source,
                          uint32_t* d_target, float* d_distances, float* d_edge_weight, float* d_mean, void* d_ws,
                          int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(k >= 1 && k <= PT_K_MAX && k_adj >= 1 && k_adj <= k, "1 <= k_adj <= k <= 64");
  WSIS_REQUIRE(V >= 1 && V < ((int64_t)1 << 30), "V outside 1 .. 2^30 - 1");
  WSIS_REQUIRE(d_geof && d_rgb && d_nbr && d_dist2 && d_features && d_source && d_target && d_distances && d_edge_weight &&
                   d_mean && d_ws,
               "null pointer");
  const int64_t E = V * k_adj, n_partial = ceil_div(E, PT_SUM_CHUNK);
  WSIS_REQUIRE(wsis_pt_edge_features_workspace_bytes(V, k_adj) <= ws_bytes, "workspace too small");
  double* partial = static_cast<double*>(d_ws);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(pt_edge_dist_kernel, dim3(grid_for(E, PT_BLOCK)), dim3(PT_BLOCK), 0, st, d_nbr, d_dist2, V, (int)k,
                     (int)k_adj, d_distances, d_source, d_target);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pt_edge_partial_kernel, dim3((unsigned)ceil_div(n_partial, PT_BLOCK)), dim3(PT_BLOCK), 0, st,
                     d_distances, E, n_partial, partial);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pt_edge_mean_kernel, dim3(1), dim3(64), 0, st, partial, n_partial, E, d_mean);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pt_edge_weight_kernel, dim3(grid_for(E, PT_BLOCK)), dim3(PT_BLOCK), 0, st, d_distances, E, d_mean,
                     lambda, d_edge_weight);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pt_features_kernel, dim3(grid_for(V, PT_BLOCK)), dim3(PT_BLOCK), 0, st, d_geof, d_rgb, V, d_features);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
