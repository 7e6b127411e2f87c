// RANSAC plane scoring for the S3DIS wall split: utils/planeSegment.py:29-63 of the reference, which calls open3d's
// PointCloud.segment_plane(distance, 3, iter) once per wall [UPSTREAM open3d].
//
// One segment_plane call draws `iter` 3-point planes and keeps the one with the most points closer than `distance`
// (ties: the smaller inlier RMSE).  That is H x N independent point-to-plane tests with one (count, sum of squares)
// reduction per plane.  wsis_plane_score does all H planes in ONE pass over the points: a lane keeps 8 points in
// registers as fp64, the workgroup walks the planes (staged in LDS, 128 at a time), and per plane
//   - the lane adds the squared distances of its own inliers (fixed order j = 0..7),
//   - the wave counts inliers with one ballot + popcount per point (scalar side, exact),
//   - one fixed-order xor butterfly sums the 64 lane values, so the cross-lane traffic is paid once per 512 points.
// Four planes go through these steps together, so that their butterflies' round trips overlap.
// The four waves' rows are added in wave order and the workgroup writes ONE (count, sum) row per plane to a slab in the
// caller's workspace; a second launch adds the slab rows in row order (the weight gradients finish the same way).  No
// floating-point atomic anywhere, and the grid is a function of (N, H) alone: the sums are bit-reproducible.
//
// The distance is |((a*x + b*y) + c*z) + d| with x, y, z widened to fp64, evaluated in that order without contraction
// (-ffp-contract=off), i.e. bit for bit what the same expression gives element-wise in numpy: `dist < thr` selects the
// same points on both sides and the counts are exact.  NaN compares false, +-inf is not below thr: a non-finite
// coordinate is never an inlier, and its square never enters a sum (select, not multiply-by-mask).
#include "common.h"

using namespace wsis;

namespace {

constexpr int PL_BLOCK = 256;                    // 4 waves
constexpr int PL_WAVES = PL_BLOCK / 64;
constexpr int PL_PTS = 8;                        // points per lane: 24 fp64 values = 48 VGPRs
constexpr int PL_TILE = PL_BLOCK * PL_PTS;       // points per workgroup = per slab row
constexpr int PL_HC = 128;                       // planes staged in LDS at a time
constexpr int PL_HMAX = 1024;
constexpr int PL_HK = 4;                         // planes whose wave reductions are in flight together
constexpr int PL_RED_SEGS = 8;                   // row segments of the slab sum (fixed: part of the order of additions)

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int64_t plane_rows(int64_t N) { return ceil_div(N, PL_TILE); }

__device__ __forceinline__ double plane_dist(double a, double b, double c, double d, double x, double y, double z) {
  return fabs(((a * x + b * y) + c * z) + d);
}

// K consecutive planes against the wave's 512 points.  Per plane the arithmetic and its order do not depend on K: K > 1
// only lets the K butterflies' cross-lane round trips overlap.
template <int K>
__device__ __forceinline__ void score_planes(const double* __restrict__ plane, const double (&px)[PL_PTS],
                                             const double (&py)[PL_PTS], const double (&pz)[PL_PTS], double thr, int lane,
                                             double* __restrict__ sum_row, int32_t* __restrict__ cnt_row) {
  double s[K];
  int cnt[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double a = plane[4 * k], b = plane[4 * k + 1], c = plane[4 * k + 2], d = plane[4 * k + 3];
    s[k] = 0.0;
    cnt[k] = 0;
#pragma unroll
    for (int j = 0; j < PL_PTS; ++j) {
      const double dist = plane_dist(a, b, c, d, px[j], py[j], pz[j]);
      const bool inl = dist < thr;
      cnt[k] += __popcll(__ballot(inl));
      s[k] += inl ? dist * dist : 0.0;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {             // both partners add the same pair: all lanes agree
    double t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = __shfl_xor(s[k], m);
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += t[k];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      sum_row[k] = s[k];
      cnt_row[k] = cnt[k];
    }
  }
}

__global__ __launch_bounds__(PL_BLOCK) void plane_score_kernel(const float* __restrict__ xyz, int64_t N,
                                                               const double* __restrict__ planes, int H, double thr,
                                                               double* __restrict__ slab_sum,
                                                               int32_t* __restrict__ slab_cnt) {
  __shared__ double s_plane[PL_HC * 4];
  __shared__ double s_sum[PL_WAVES][PL_HC];
  __shared__ int32_t s_cnt[PL_WAVES][PL_HC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * PL_TILE + (int64_t)wave * (64 * PL_PTS) + lane;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double px[PL_PTS], py[PL_PTS], pz[PL_PTS];
#pragma unroll
  for (int j = 0; j < PL_PTS; ++j) {
    const int64_t i = base + (int64_t)j * 64;
    const bool in_range = i < N;                 // a point past the end is NaN: never an inlier
    px[j] = in_range ? (double)xyz[3 * i] : qnan;
    py[j] = in_range ? (double)xyz[3 * i + 1] : qnan;
    pz[j] = in_range ? (double)xyz[3 * i + 2] : qnan;
  }
  for (int h0 = 0; h0 < H; h0 += PL_HC) {
    const int hc = min(PL_HC, H - h0);
    __syncthreads();                             // the previous chunk's rows have been read
    for (int t = tid; t < hc * 4; t += PL_BLOCK) s_plane[t] = planes[(int64_t)h0 * 4 + t];
    __syncthreads();
    int hh = 0;
    for (; hh + PL_HK <= hc; hh += PL_HK)
      score_planes<PL_HK>(s_plane + 4 * hh, px, py, pz, thr, lane, &s_sum[wave][hh], &s_cnt[wave][hh]);
    for (; hh < hc; ++hh) score_planes<1>(s_plane + 4 * hh, px, py, pz, thr, lane, &s_sum[wave][hh], &s_cnt[wave][hh]);
    __syncthreads();
    if (tid < hc) {
      double s = s_sum[0][tid];
      int32_t cnt = s_cnt[0][tid];
#pragma unroll
      for (int w = 1; w < PL_WAVES; ++w) {
        s += s_sum[w][tid];
        cnt += s_cnt[w][tid];
      }
      const int64_t o = (int64_t)blockIdx.x * H + h0 + tid;
      slab_sum[o] = s;
      slab_cnt[o] = cnt;
    }
  }
}

// rows of the slab added in row order: segment g of PL_RED_SEGS takes rows [R*g/8, R*(g+1)/8) one after the other,
// the eight segment sums are added in segment order
__global__ __launch_bounds__(64 * PL_RED_SEGS) void plane_slab_sum_kernel(const double* __restrict__ slab_sum,
                                                                          const int32_t* __restrict__ slab_cnt,
                                                                          int64_t R, int H, int64_t* __restrict__ count,
                                                                          double* __restrict__ sumsq) {
  __shared__ double s_sum[PL_RED_SEGS][64];
  __shared__ int64_t s_cnt[PL_RED_SEGS][64];
  const int l = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int h = blockIdx.x * 64 + l;
  double s = 0.0;
  int64_t c = 0;
  if (h < H) {
    const int64_t r1 = R * (g + 1) / PL_RED_SEGS;
    for (int64_t r = R * g / PL_RED_SEGS; r < r1; ++r) {
      s += slab_sum[r * H + h];
      c += slab_cnt[r * H + h];
    }
  }
  s_sum[g][l] = s;
  s_cnt[g][l] = c;
  __syncthreads();
  if (g == 0 && h < H) {
#pragma unroll
    for (int k = 1; k < PL_RED_SEGS; ++k) {
      s += s_sum[k][l];
      c += s_cnt[k][l];
    }
    count[h] = c;
    sumsq[h] = s;
  }
}

__global__ void plane_mark_kernel(const float* __restrict__ xyz, int64_t N, const double* __restrict__ plane4, double thr,
                                  uint8_t* __restrict__ mask) {
  const double a = plane4[0], b = plane4[1], c = plane4[2], d = plane4[3];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const double dist = plane_dist(a, b, c, d, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]);
    mask[i] = dist < thr ? 1 : 0;
  }
}

}  // namespace

extern "C" {

int64_t wsis_plane_score_workspace_bytes(int64_t N, int32_t H) {
  if (N < 0 || H < 1 || H > PL_HMAX) return -1;
  const int64_t R = plane_rows(N);
  return (int64_t)(align256((size_t)R * H * sizeof(double)) + align256((size_t)R * H * sizeof(int32_t)) + 256);
}

int wsis_plane_score(const float* d_xyz, int64_t N, const double* d_planes, int32_t H, double thr, int64_t* d_count,
                     double* d_sumsq, void* d_ws, int64_t ws_bytes, void* stream) {
  WSIS_REQUIRE(N >= 0, "N < 0");
  WSIS_REQUIRE(H >= 1 && H <= PL_HMAX, "H outside [1, 1024]: score more hypotheses in several calls");
  hipStream_t st = as_stream(stream);
  if (N == 0) {                                  // zeros, no launch
    if (d_count) WSIS_HIP_CHECK(hipMemsetAsync(d_count, 0, (size_t)H * sizeof(int64_t), st));
    if (d_sumsq) WSIS_HIP_CHECK(hipMemsetAsync(d_sumsq, 0, (size_t)H * sizeof(double), st));
    return WSIS_OK;
  }
  WSIS_REQUIRE(d_xyz && d_planes && d_count && d_sumsq, "null pointer");
  const int64_t R = plane_rows(N);
  WSIS_REQUIRE(R <= 0x7fffffff, "N too large for one launch");
  WSIS_REQUIRE(d_ws && ws_bytes >= wsis_plane_score_workspace_bytes(N, H), "workspace too small");
  double* slab_sum = static_cast<double*>(d_ws);
  int32_t* slab_cnt = reinterpret_cast<int32_t*>(static_cast<char*>(d_ws) + align256((size_t)R * H * sizeof(double)));
  hipLaunchKernelGGL(plane_score_kernel, dim3((unsigned)R), dim3(PL_BLOCK), 0, st, d_xyz, N, d_planes, (int)H, thr,
                     slab_sum, slab_cnt);
  WSIS_LAUNCH_CHECK();
  hipLaunchKernelGGL(plane_slab_sum_kernel, dim3((unsigned)ceil_div(H, 64)), dim3(64 * PL_RED_SEGS), 0, st, slab_sum,
                     slab_cnt, R, (int)H, d_count, d_sumsq);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_plane_mark(const float* d_xyz, int64_t N, const double* d_plane4, double thr, uint8_t* d_mask, void* stream) {
  WSIS_REQUIRE(N >= 0, "N < 0");
  if (N == 0) return WSIS_OK;
  WSIS_REQUIRE(d_xyz && d_plane4 && d_mask, "null pointer");
  hipLaunchKernelGGL(plane_mark_kernel, dim3(grid_for(N, 256)), dim3(256), 0, as_stream(stream), d_xyz, N, d_plane4, thr,
                     d_mask);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
