// Building the superpoint graph of a scene (data/ScanNetV2/prepare_data_inst_ScanNetV2.py and
// data/S3DIS/prepare_S3DIS_inst_data.py of the reference), the per-point and per-pair parts:
//
//   compute_edges_feature, superpoint half    ScanNet :359-394 / S3DIS :287-322    wsis_gp_sp_moments
//   stats.mode of the labels of a superpoint  ScanNet :241-249 / S3DIS :173-183    wsis_gp_label_mode
//   KDTree.query_radius / KDTree.query        ScanNet :213-215 / S3DIS :141-156    wsis_gp_neighbors
//   compute_edges_feature, edge half          ScanNet :398-426 / S3DIS :325-354    wsis_gp_edge_features
//
// The reference forms one `np.where(superpoint == spID)` mask per superpoint and per use: O(S*N).  Here every kernel
// walks the point CSR of the superpoints (wsis_segment_csr: the permutation is stable, a row lists its points in
// ascending index order, which is the order of xyz[np.where(superpoint == spID)[0]]); one wave owns one row, one
// query or one edge.
//
// Reproducibility: no floating-point atomic.  Every sum is taken by the lanes of one wave in a fixed lane-strided
// order and finished by one xor butterfly, in which both partners add the same pair: every lane ends with the same
// value and two calls give the same bytes.  Products and sums stay uncontracted (-ffp-contract=off).
#include "common.h"

using namespace wsis;

namespace {

constexpr int GP_BLOCK = 256;
constexpr int GP_WAVES = GP_BLOCK / 64;
constexpr int GP_K_MAX = 128;
constexpr int GP_SWEEPS = 12;                    // cyclic Jacobi on a 3x3 converges quadratically: 5-6 sweeps in practice

__device__ __forceinline__ double gp_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

__device__ __forceinline__ double gp_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ int gp_wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ int gp_wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}

// one Jacobi rotation that annihilates a_pq; r is the third index: a_rp, a_rq are the other two off-diagonal entries
__device__ __forceinline__ void gp_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
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
}

// eigenvalues of the symmetric 3x3 (xx, yy, zz, xy, xz, yz), descending
__device__ __forceinline__ void gp_eig3(double xx, double yy, double zz, double xy, double xz, double yz, double* ev) {
  for (int sweep = 0; sweep < GP_SWEEPS; ++sweep) {
    const double off = fabs(xy) + fabs(xz) + fabs(yz);
    if (off == 0.0 || off <= 1e-300 + 1e-22 * (fabs(xx) + fabs(yy) + fabs(zz))) break;
    gp_rotate(xx, yy, xy, xz, yz);               // (p, q) = (x, y), r = z
    gp_rotate(xx, zz, xz, xy, yz);               // (p, q) = (x, z), r = y: a_rp = xy, a_rq = yz
    gp_rotate(yy, zz, yz, xy, xz);               // (p, q) = (y, z), r = x: a_rp = xy, a_rq = xz
  }
  double a = xx, b = yy, c = zz, t;
  if (a < b) { t = a; a = b; b = t; }
  if (b < c) { t = b; b = c; c = t; }
  if (a < b) { t = a; a = b; b = t; }
  ev[0] = a;
  ev[1] = b;
  ev[2] = c;
}

// ---- per-superpoint moments and the three shape features
__global__ __launch_bounds__(GP_BLOCK) void gp_sp_moments_kernel(
    const float* __restrict__ xyz, const int32_t* __restrict__ perm, const int32_t* __restrict__ offsets, int64_t N,
    int64_t S, int64_t* __restrict__ count, float* __restrict__ centroid, float* __restrict__ length,
    float* __restrict__ surface, float* __restrict__ volume, double* __restrict__ cov6, double* __restrict__ ev3) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * GP_WAVES + (threadIdx.x >> 6);
  if (s >= S) return;                            // wave-uniform
  const int b = offsets[s], e = offsets[s + 1];
  const int n = e - b;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = b + lane; j < e; j += 64) {
    const int64_t p = perm[j];
    if (p < 0 || p >= N) continue;
    sx += (double)xyz[3 * p];
    sy += (double)xyz[3 * p + 1];
    sz += (double)xyz[3 * p + 2];
  }
  sx = gp_wave_sum(sx);
  sy = gp_wave_sum(sy);
  sz = gp_wave_sum(sz);
  const double dn = (double)n;
  const double mx = n > 0 ? sx / dn : 0.0, my = n > 0 ? sy / dn : 0.0, mz = n > 0 ? sz / dn : 0.0;
  double cxx = 0.0, cyy = 0.0, czz = 0.0, cxy = 0.0, cxz = 0.0, cyz = 0.0;
  for (int j = b + lane; j < e; j += 64) {
    const int64_t p = perm[j];
    if (p < 0 || p >= N) continue;
    const double dx = (double)xyz[3 * p] - mx, dy = (double)xyz[3 * p + 1] - my, dz = (double)xyz[3 * p + 2] - mz;
    cxx += dx * dx;
    cyy += dy * dy;
    czz += dz * dz;
    cxy += dx * dy;
    cxz += dx * dz;
    cyz += dy * dz;
  }
  cxx = gp_wave_sum(cxx);
  cyy = gp_wave_sum(cyy);
  czz = gp_wave_sum(czz);
  cxy = gp_wave_sum(cxy);
  cxz = gp_wave_sum(cxz);
  cyz = gp_wave_sum(cyz);
  double ev[3] = {0.0, 0.0, 0.0};
  double len = 0.0, sur = 0.0, vol = 0.0;
  if (n >= 3) {                                  // np.cov divides by n - 1
    const double d = dn - 1.0;
    cxx /= d;
    cyy /= d;
    czz /= d;
    cxy /= d;
    cxz /= d;
    cyz /= d;
    gp_eig3(cxx, cyy, czz, cxy, cxz, cyz, ev);
    len = ev[0];
    sur = sqrt(ev[0] * ev[1] + 1e-10);
    vol = sqrt(ev[0] * ev[1] * ev[2] + 1e-10);
  } else if (n == 2) {                           // np.var: the population variance
    cxx /= dn;
    cyy /= dn;
    czz /= dn;
    cxy /= dn;
    cxz /= dn;
    cyz /= dn;
    len = sqrt((cxx + cyy) + czz);
  }
  if (lane == 0) {
    count[s] = n;
    centroid[3 * s] = (float)mx;
    centroid[3 * s + 1] = (float)my;
    centroid[3 * s + 2] = (float)mz;
    length[s] = (float)len;
    surface[s] = (float)sur;
    volume[s] = (float)vol;
    if (cov6) {
      cov6[6 * s] = cxx;
      cov6[6 * s + 1] = cyy;
      cov6[6 * s + 2] = czz;
      cov6[6 * s + 3] = cxy;
      cov6[6 * s + 4] = cxz;
      cov6[6 * s + 5] = cyz;
    }
    if (ev3) {
      ev3[3 * s] = ev[0];
      ev3[3 * s + 1] = ev[1];
      ev3[3 * s + 2] = ev[2];
    }
  }
}

// ---- the most frequent label rank of every row; the smallest rank wins a tie.  Ranks are dense and ascending in the
// label value, so "smallest rank" is stats.mode's "smallest value".  Each round takes the smallest rank above the last
// one counted (a wave minimum over the row) and counts it over the row, 64 points per ballot.
__global__ __launch_bounds__(GP_BLOCK) void gp_label_mode_kernel(const int32_t* __restrict__ rank,
                                                                 const int32_t* __restrict__ perm,
                                                                 const int32_t* __restrict__ offsets, int64_t N, int64_t S,
                                                                 int32_t* __restrict__ mode, int32_t* __restrict__ mode_count) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * GP_WAVES + (threadIdx.x >> 6);
  if (s >= S) return;
  const int b = offsets[s], e = offsets[s + 1];
  const int n = e - b;
  int last = -1, best = -1, best_n = 0, seen = 0;
  while (seen < n) {                             // wave-uniform: every value is the result of a wave reduction
    int cur = 0x7fffffff;
    for (int j = b + lane; j < e; j += 64) {
      const int64_t p = perm[j];
      const int r = (p >= 0 && p < N) ? rank[p] : -1;
      if (r > last) cur = min(cur, r);
    }
    cur = gp_wave_min(cur);
    if (cur == 0x7fffffff) break;                // only ranks below zero are left: not labels
    int c = 0;
    for (int j0 = b; j0 < e; j0 += 64) {
      const int j = j0 + lane;
      bool hit = false;
      if (j < e) {
        const int64_t p = perm[j];
        hit = p >= 0 && p < N && rank[p] == cur;
      }
      c += __popcll(__ballot(hit));
    }
    if (c > best_n) {                            // strict: the earlier (smaller) rank keeps a tie
      best_n = c;
      best = cur;
    }
    seen += c;
    last = cur;
    if (best_n >= n - seen) break;               // what is left cannot beat it (a tie goes to the smaller rank)
  }
  if (lane == 0) {
    mode[s] = best;
    mode_count[s] = best_n;
  }
}

// ---- neighbour lists: one wave per query, brute force over the S centres.  Round r takes the smallest (d2, id) pair
// strictly above the pair of round r - 1: a total order, so the list does not depend on how the lanes are dealt.
struct GpPair {
  double d;
  int id;
};
__device__ __forceinline__ bool gp_less(double d0, int i0, double d1, int i1) { return d0 < d1 || (d0 == d1 && i0 < i1); }

__global__ __launch_bounds__(GP_BLOCK) void gp_neighbors_kernel(const float* __restrict__ centres, int64_t S, int k,
                                                                double radius2, int32_t* __restrict__ nbr,
                                                                double* __restrict__ dist2, int32_t* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * GP_WAVES + (threadIdx.x >> 6);
  if (q >= S) return;
  const double qx = (double)centres[3 * q], qy = (double)centres[3 * q + 1], qz = (double)centres[3 * q + 2];
  const int iS = (int)S;
  double last_d = -1.0;                          // below every distance
  int last_i = -1;
  int found = k;
  for (int r = 0; r < k; ++r) {
    double bd = gp_inf();
    int bi = 0x7fffffff;
    int within = 0;
    for (int i = lane; i < iS; i += 64) {
      if (i == (int)q) continue;
      const double dx = (double)centres[3 * i] - qx, dy = (double)centres[3 * i + 1] - qy,
                   dz = (double)centres[3 * i + 2] - qz;
      const double d = (dx * dx + dy * dy) + dz * dz;
      if (!(d <= radius2)) continue;
      if (r == 0) ++within;                       // the count of the radius is taken once, in the first round
      if (gp_less(last_d, last_i, d, i) && gp_less(d, i, bd, bi)) {
        bd = d;
        bi = i;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double od = __shfl_xor(bd, m);
      const int oi = __shfl_xor(bi, m);
      if (gp_less(od, oi, bd, bi)) {
        bd = od;
        bi = oi;
      }
    }
    if (r == 0) {
      within = gp_wave_sum(within);
      if (lane == 0) count[q] = within;
    }
    if (bi == 0x7fffffff) {                      // wave-uniform: the list ends here
      found = r;
      break;
    }
    if (lane == 0) {
      nbr[q * k + r] = bi;
      dist2[q * k + r] = bd;
    }
    last_d = bd;
    last_i = bi;
  }
  for (int r = found + lane; r < k; r += 64) {
    nbr[q * k + r] = -1;
    dist2[q * k + r] = gp_inf();
  }
}

// ---- the 13 features of a directed edge (s, t): one wave per edge
__global__ __launch_bounds__(GP_BLOCK) void gp_edge_features_kernel(
    const float* __restrict__ xyz, const int32_t* __restrict__ perm, const int32_t* __restrict__ offsets, int64_t N,
    int64_t S, const int64_t* __restrict__ edges, int64_t E, const int64_t* __restrict__ samp_off,
    const int32_t* __restrict__ samp, const float* __restrict__ centroid, const float* __restrict__ length,
    const float* __restrict__ surface, const float* __restrict__ volume, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t ei = (int64_t)blockIdx.x * GP_WAVES + (threadIdx.x >> 6);
  if (ei >= E) return;
  const int64_t s = edges[2 * ei], t = edges[2 * ei + 1];
  float* __restrict__ o = out + 13 * ei;
  const float qnan = __int_as_float(0x7fc00000);
  if (s < 0 || s >= S || t < 0 || t >= S) {      // refused on the host; never read outside the tables
    if (lane < 13) o[lane] = qnan;
    return;
  }
  const int bs = offsets[s], ns = offsets[s + 1] - bs, bt = offsets[t], nt = offsets[t + 1] - bt;
  const int m = min(ns, nt), big = max(ns, nt);
  const int64_t so = samp_off[ei];
  const bool sampled = ns != nt;
  if (sampled && samp_off[ei + 1] - so != m) {
    if (lane < 13) o[lane] = qnan;
    return;
  }
  // pair j: (point j of the smaller row, point samp[j] of the larger row); (j, j) for rows of equal length
  auto delta = [&](int j, float* d) {
    int js = j, jt = j;
    if (sampled) {
      int k = samp[so + j];
      k = k < 0 ? 0 : (k >= big ? big - 1 : k);
      if (ns > nt) js = k; else jt = k;
    }
    int64_t ps = perm[bs + js], pt = perm[bt + jt];
    ps = ps < 0 ? 0 : (ps >= N ? N - 1 : ps);
    pt = pt < 0 ? 0 : (pt >= N ? N - 1 : pt);
    d[0] = xyz[3 * ps] - xyz[3 * pt];            // fp32, as numpy subtracts two float32 arrays
    d[1] = xyz[3 * ps + 1] - xyz[3 * pt + 1];
    d[2] = xyz[3 * ps + 2] - xyz[3 * pt + 2];
  };
  float mean[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
  if (m == 1) {
    float d[3];
    delta(0, d);
    mean[0] = d[0];
    mean[1] = d[1];
    mean[2] = d[2];
  } else if (m > 1) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int j = lane; j < m; j += 64) {
      float d[3];
      delta(j, d);
      a0 += (double)d[0];
      a1 += (double)d[1];
      a2 += (double)d[2];
    }
    const double dm = (double)m;
    const double m0 = gp_wave_sum(a0) / dm, m1 = gp_wave_sum(a1) / dm, m2 = gp_wave_sum(a2) / dm;
    a0 = a1 = a2 = 0.0;
    for (int j = lane; j < m; j += 64) {
      float d[3];
      delta(j, d);
      const double e0 = (double)d[0] - m0, e1 = (double)d[1] - m1, e2 = (double)d[2] - m2;
      a0 += e0 * e0;
      a1 += e1 * e1;
      a2 += e2 * e2;
    }
    mean[0] = (float)m0;
    mean[1] = (float)m1;
    mean[2] = (float)m2;
    sd[0] = (float)sqrt(gp_wave_sum(a0) / dm);
    sd[1] = (float)sqrt(gp_wave_sum(a1) / dm);
    sd[2] = (float)sqrt(gp_wave_sum(a2) / dm);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      o[j] = mean[j];
      o[3 + j] = sd[j];
      o[6 + j] = centroid[3 * s + j] - centroid[3 * t + j];
    }
    o[9] = length[s] / (length[t] + 1e-6f);
    o[10] = surface[s] / (surface[t] + 1e-6f);
    o[11] = volume[s] / (volume[t] + 1e-6f);
    o[12] = (float)((double)ns / ((double)nt + 1e-6));
  }
}

}  // namespace

extern "C" {

int wsis_gp_sp_moments(const float* d_xyz, const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t S,
                       int64_t* d_count, float* d_centroid, float* d_length, float* d_surface, float* d_volume,
                       double* d_cov6, double* d_ev3, void* stream) {
  WSIS_REQUIRE(N >= 0 && S >= 0, "negative size");
  WSIS_REQUIRE(N < ((int64_t)1 << 31), "N too large for the int32 CSR");
  if (S == 0) return WSIS_OK;
  WSIS_REQUIRE(d_offsets && d_count && d_centroid && d_length && d_surface && d_volume && (N == 0 || (d_xyz && d_perm)),
               "null pointer");
  const int64_t g = ceil_div(S, GP_WAVES);
  WSIS_REQUIRE(g <= 0x7fffffff, "S too large for one launch");
  hipLaunchKernelGGL(gp_sp_moments_kernel, dim3((unsigned)g), dim3(GP_BLOCK), 0, as_stream(stream), d_xyz, d_perm,
                     d_offsets, N, S, d_count, d_centroid, d_length, d_surface, d_volume, d_cov6, d_ev3);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_gp_label_mode(const int32_t* d_rank, const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t S,
                       int32_t* d_mode, int32_t* d_mode_count, void* stream) {
  WSIS_REQUIRE(N >= 0 && S >= 0, "negative size");
  WSIS_REQUIRE(N < ((int64_t)1 << 31), "N too large for the int32 CSR");
  if (S == 0) return WSIS_OK;
  WSIS_REQUIRE(d_offsets && d_mode && d_mode_count && (N == 0 || (d_rank && d_perm)), "null pointer");
  const int64_t g = ceil_div(S, GP_WAVES);
  WSIS_REQUIRE(g <= 0x7fffffff, "S too large for one launch");
  hipLaunchKernelGGL(gp_label_mode_kernel, dim3((unsigned)g), dim3(GP_BLOCK), 0, as_stream(stream), d_rank, d_perm,
                     d_offsets, N, S, d_mode, d_mode_count);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_gp_neighbors(const float* d_centres, int64_t S, int32_t k, double radius, int32_t* d_nbr, double* d_dist2,
                      int32_t* d_count, void* stream) {
  WSIS_REQUIRE(S >= 0, "negative size");
  WSIS_REQUIRE(S < ((int64_t)1 << 31) / GP_K_MAX, "S too large for int32 indices");
  WSIS_REQUIRE(k >= 1 && k <= GP_K_MAX, "1 <= k <= 128");
  WSIS_REQUIRE(radius >= 0.0, "radius < 0 (or NaN)");
  if (S == 0) return WSIS_OK;
  WSIS_REQUIRE(d_centres && d_nbr && d_dist2 && d_count, "null pointer");
  hipLaunchKernelGGL(gp_neighbors_kernel, dim3((unsigned)ceil_div(S, GP_WAVES)), dim3(GP_BLOCK), 0, as_stream(stream),
                     d_centres, S, (int)k, radius * radius, d_nbr, d_dist2, d_count);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_gp_edge_features(const float* d_xyz, const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t S,
                          const int64_t* d_edges, int64_t E, const int64_t* d_samp_off, const int32_t* d_samp,
                          const float* d_centroid, const float* d_length, const float* d_surface, const float* d_volume,
                          float* d_out, void* stream) {
  WSIS_REQUIRE(N >= 0 && S >= 0 && E >= 0, "negative size");
  WSIS_REQUIRE(N < ((int64_t)1 << 31), "N too large for the int32 CSR");
  if (E == 0) return WSIS_OK;
  WSIS_REQUIRE(N > 0 && S > 0, "edges without points");
  WSIS_REQUIRE(d_xyz && d_perm && d_offsets && d_edges && d_samp_off && d_centroid && d_length && d_surface && d_volume &&
                   d_out,
               "null pointer");
  const int64_t g = ceil_div(E, GP_WAVES);
  WSIS_REQUIRE(g <= 0x7fffffff, "E too large for one launch");
  hipLaunchKernelGGL(gp_edge_features_kernel, dim3((unsigned)g), dim3(GP_BLOCK), 0, as_stream(stream), d_xyz, d_perm,
                     d_offsets, N, S, d_edges, E, d_samp_off, d_samp, d_centroid, d_length, d_surface, d_volume, d_out);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
