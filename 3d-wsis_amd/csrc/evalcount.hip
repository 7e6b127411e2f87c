// The counting behind the three evaluators of the reference (evaluation/basic/ins_seg_evaluator.py:70-115,
// utils/eval_s3dis.py:50-112, evaluation/basic/sem_seg_evaluator.py:34-37, used by test_scannetv2.py:133-143, 212-275,
// test_s3dis.py:135-148, 216-292 and do_validation of train_scannetv2.py:296-400):
//
//   wsis_mask_overlap   T[p, u] = #{i : mask[p, i] != 0 and col[i] == u}, rows[p] = #{i : mask[p, i] != 0}
//   wsis_label_pairs    T[a, b] = #{i : a_i == a and b_i == b}
//
// The reference evaluates one `np.logical_and(gt_ids == id, pred_mask)` per (prediction, ground-truth instance):
// O(instances * N) per prediction.  Here the [P, N] masks are read ONCE.  Lanes run along the points; a workgroup owns
// EC_CHUNK points and a tile of R(G) mask rows whose R x G int32 counters live in LDS.  The columns of the chunk are read
// once into registers.  Per row and 64 points one ballot says which lanes are members (no member: the wave moves on --
// masks are sparse, a point belongs to about one prediction); the member lanes are then grouped by column with one
// ballot per DISTINCT column and one lane adds the popcount to LDS: members of a prediction fall into one or two
// ground-truth instances, where per-lane LDS atomics would all hit one address.  At the end of the chunk the non-zero
// counters go to the int64 table in global memory with integer atomics.  Integers only: the result is exact and does
// not depend on the order of arrival; the grid is a function of (P, N, G) alone.
#include "common.h"

using namespace wsis;

namespace {

constexpr int EC_BLOCK = 256;                    // 4 waves
constexpr int EC_PTS = 8;                        // points per lane whose column stays in a register
constexpr int EC_CHUNK = EC_BLOCK * EC_PTS;      // points per workgroup
constexpr int EC_WAVE_PTS = 64 * EC_PTS;         // consecutive points of one wave
constexpr int EC_LDS = 4096;                     // int32 counters per workgroup (16 KiB: ~10 workgroups share a CU)
constexpr int EC_RMAX = 32;                      // rows of a tile at most
constexpr int EC_GMAX = 4096;
constexpr int EC_PAIRS_MAX = 65536;

inline int tile_rows(int G) {
  const int r = EC_LDS / G;
  return r < 1 ? 1 : (r > EC_RMAX ? EC_RMAX : r);
}

// Adds, for every distinct key among the lanes with `active`, the number of such lanes to cnt[key]: the first pending
// lane's key is broadcast, one ballot finds the lanes that share it, that first lane adds their count.  Every lane of the
// wave must call it (the loop condition is wave-uniform); the caller guarantees 0 <= key < size of cnt for active lanes.
__device__ __forceinline__ void add_by_key(int32_t* cnt, int key, bool active, int lane) {
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int lead = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const int k = __builtin_amdgcn_readlane(key, lead);
    const unsigned long long same = __ballot(active && key == k);
    if (lane == lead) atomicAdd(cnt + k, (int32_t)__popcll(same));
    todo &= ~same;
  }
}

// the same straight to a global int64 table (tables too large for LDS)
__device__ __forceinline__ void add_by_key_global(unsigned long long* cnt, int key, bool active, int lane) {
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int lead = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const int k = __builtin_amdgcn_readlane(key, lead);
    const unsigned long long same = __ballot(active && key == k);
    if (lane == lead) atomicAdd(cnt + k, (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

// grid (chunks, row tiles).  E = uint8_t or unsigned long long: a member is an element with ANY bit set.
template <typename E>
__global__ __launch_bounds__(EC_BLOCK) void mask_overlap_kernel(const E* __restrict__ mask, int64_t P, int64_t N,
                                                                const int32_t* __restrict__ col, int G, int R,
                                                                unsigned long long* __restrict__ table,
                                                                unsigned long long* __restrict__ rows) {
  __shared__ int32_t s_cnt[EC_LDS];
  __shared__ int32_t s_rows[EC_RMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.y * R;
  const int nr = (int)(P - row0 < R ? P - row0 : R);         // rows of this tile: nr * G <= EC_LDS
  for (int t = tid; t < nr * G; t += EC_BLOCK) s_cnt[t] = 0;
  if (tid < EC_RMAX) s_rows[tid] = 0;
  const int64_t base = (int64_t)blockIdx.x * EC_CHUNK + (int64_t)wave * EC_WAVE_PTS + lane;
  // a point past the end reads the last point instead (N >= 1 here) and is masked out: no branch around a load, so
  // the eight loads of a row are in flight together
  int64_t at[EC_PTS];
  int c[EC_PTS];
  unsigned inside = 0;
#pragma unroll
  for (int j = 0; j < EC_PTS; ++j) {
    const int64_t i = base + (int64_t)j * 64;
    inside |= (i < N ? 1u : 0u) << j;
    at[j] = i < N ? i : N - 1;
  }
#pragma unroll
  for (int j = 0; j < EC_PTS; ++j) {
    const int v = col[at[j]];
    c[j] = ((inside >> j & 1u) && v >= 0 && v < G) ? v : -1;  // outside [0, G): counts in rows only
  }
  __syncthreads();
  for (int r = 0; r < nr; ++r) {
    const E* __restrict__ m = mask + (row0 + r) * N;
    E v[EC_PTS];
#pragma unroll
    for (int j = 0; j < EC_PTS; ++j) v[j] = m[at[j]];
    int members = 0;
#pragma unroll
    for (int j = 0; j < EC_PTS; ++j) {
      const bool in = v[j] != (E)0 && (inside >> j & 1u);
      const unsigned long long b = __ballot(in);
      if (b == 0) continue;                                  // wave-uniform
      members += __popcll(b);
      add_by_key(s_cnt + r * G, c[j], in && c[j] >= 0, lane);
    }
    if (lane == 0 && members) atomicAdd(s_rows + r, members);
  }
  __syncthreads();
  for (int t = tid; t < nr * G; t += EC_BLOCK) {             // rows of a tile are consecutive in the table
    const int32_t n = s_cnt[t];
    if (n) atomicAdd(table + row0 * G + t, (unsigned long long)n);
  }
  if (tid < nr && s_rows[tid]) atomicAdd(rows + row0 + tid, (unsigned long long)s_rows[tid]);
}

// A * B <= EC_LDS: per-workgroup int32 table in LDS, flushed once (a workgroup sees fewer than 2^31 points)
__global__ __launch_bounds__(EC_BLOCK) void label_pairs_lds_kernel(const int32_t* __restrict__ a,
                                                                   const int32_t* __restrict__ b, int64_t N, int A, int B,
                                                                   unsigned long long* __restrict__ table) {
  __shared__ int32_t s_cnt[EC_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int T = A * B;
  for (int t = tid; t < T; t += EC_BLOCK) s_cnt[t] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * EC_BLOCK;
  for (int64_t i0 = (int64_t)blockIdx.x * EC_BLOCK + (tid - lane); i0 < N; i0 += stride) {     // wave-uniform
    const int64_t i = i0 + lane;
    int key = -1;
    if (i < N) {
      const int x = a[i], y = b[i];
      if (x >= 0 && x < A && y >= 0 && y < B) key = x * B + y;
    }
    add_by_key(s_cnt, key, key >= 0, lane);
  }
  __syncthreads();
  for (int t = tid; t < T; t += EC_BLOCK) {
    const int32_t n = s_cnt[t];
    if (n) atomicAdd(table + t, (unsigned long long)n);
  }
}

__global__ __launch_bounds__(EC_BLOCK) void label_pairs_global_kernel(const int32_t* __restrict__ a,
                                                                      const int32_t* __restrict__ b, int64_t N, int A,
                                                                      int B, unsigned long long* __restrict__ table) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t stride = (int64_t)gridDim.x * EC_BLOCK;
  for (int64_t i0 = (int64_t)blockIdx.x * EC_BLOCK + (tid - lane); i0 < N; i0 += stride) {     // wave-uniform
    const int64_t i = i0 + lane;
    int key = -1;
    if (i < N) {
      const int x = a[i], y = b[i];
      if (x >= 0 && x < A && y >= 0 && y < B) key = x * B + y;
    }
    add_by_key_global(table, key, key >= 0, lane);
  }
}

}  // namespace

extern "C" {

int32_t wsis_mask_overlap_chunk(void) { return EC_CHUNK; }

int32_t wsis_mask_overlap_tile_rows(int32_t G) { return (G < 1 || G > EC_GMAX) ? -1 : tile_rows(G); }

int64_t wsis_mask_overlap_workspace_bytes(int64_t P, int64_t N, int32_t G) {
  if (P < 0 || N < 0 || G < 1 || G > EC_GMAX) return -1;
  return 0;                                      // the counters live in LDS: nothing to reserve
}

int wsis_mask_overlap(const void* d_mask, int32_t elem_bytes, int64_t P, int64_t N, const int32_t* d_col, int32_t G,
                      int64_t* d_table, int64_t* d_rows, void* d_ws, int64_t ws_bytes, void* stream) {
  (void)d_ws;
  (void)ws_bytes;
  WSIS_REQUIRE(P >= 0 && N >= 0, "negative size");
  WSIS_REQUIRE(G >= 1 && G <= EC_GMAX, "G outside [1, 4096]");
  WSIS_REQUIRE(elem_bytes == 1 || elem_bytes == 8, "elem_bytes must be 1 (bool / uint8) or 8 (int64)");
  hipStream_t st = as_stream(stream);
  if (P > 0) {
    WSIS_REQUIRE(d_table && d_rows, "null pointer");
    WSIS_HIP_CHECK(hipMemsetAsync(d_table, 0, (size_t)P * G * sizeof(int64_t), st));
    WSIS_HIP_CHECK(hipMemsetAsync(d_rows, 0, (size_t)P * sizeof(int64_t), st));
  }
  if (P == 0 || N == 0) return WSIS_OK;
  WSIS_REQUIRE(d_mask && d_col, "null pointer");
  const int R = tile_rows(G);
  const int64_t chunks = ceil_div(N, EC_CHUNK), tiles = ceil_div(P, R);
  WSIS_REQUIRE(chunks <= 0x7fffffff && tiles <= 65535, "P or N too large for one launch");
  const dim3 grid((unsigned)chunks, (unsigned)tiles);
  unsigned long long* table = reinterpret_cast<unsigned long long*>(d_table);
  unsigned long long* rows = reinterpret_cast<unsigned long long*>(d_rows);
  if (elem_bytes == 1)
    hipLaunchKernelGGL(mask_overlap_kernel<uint8_t>, grid, dim3(EC_BLOCK), 0, st, static_cast<const uint8_t*>(d_mask), P,
                       N, d_col, (int)G, R, table, rows);
  else
    hipLaunchKernelGGL(mask_overlap_kernel<unsigned long long>, grid, dim3(EC_BLOCK), 0, st,
                       static_cast<const unsigned long long*>(d_mask), P, N, d_col, (int)G, R, table, rows);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_label_pairs(const int32_t* d_a, const int32_t* d_b, int64_t N, int32_t A, int32_t B, int64_t* d_table,
                     void* stream) {
  WSIS_REQUIRE(N >= 0, "N < 0");
  WSIS_REQUIRE(A >= 1 && B >= 1 && (int64_t)A * B <= EC_PAIRS_MAX, "A, B >= 1 and A * B <= 65536");
  WSIS_REQUIRE(N < ((int64_t)1 << 40), "N too large");
  WSIS_REQUIRE(d_table, "null pointer");
  hipStream_t st = as_stream(stream);
  const int T = A * B;
  WSIS_HIP_CHECK(hipMemsetAsync(d_table, 0, (size_t)T * sizeof(int64_t), st));
  if (N == 0) return WSIS_OK;
  WSIS_REQUIRE(d_a && d_b, "null pointer");
  unsigned long long* table = reinterpret_cast<unsigned long long*>(d_table);
  const int g = grid_for(N, EC_BLOCK);
  if (T <= EC_LDS)
    hipLaunchKernelGGL(label_pairs_lds_kernel, dim3(g), dim3(EC_BLOCK), 0, st, d_a, d_b, N, (int)A, (int)B, table);
  else
    hipLaunchKernelGGL(label_pairs_global_kernel, dim3(g), dim3(EC_BLOCK), 0, st, d_a, d_b, N, (int)A, (int)B, table);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
