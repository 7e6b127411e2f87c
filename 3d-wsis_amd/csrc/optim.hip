// AdamW over a table of parameter segments in ONE launch (train_scannetv2.py:251 `optimizer.step()`, optimizer from
// config/ScanNet_v2_3D_WSIS.yaml:58-61: AdamW, lr 1e-3, weight_decay 1e-4).  HBM bound: reads p, g, m, v and writes
// p, m, v = 28 bytes per parameter (11.1 M parameters -> 311 MB).  torch's multi-tensor fused AdamW hands 65,536
// elements to a 512-thread block: the 361 tensors of this model become ~85 blocks per launch in 6 launches (a third of
// the CUs, 1.3 TB/s, 233 us); here a workgroup takes 1,024 elements, every tensor in the same launch.
#include "common.h"

#include <cstddef>

namespace wsis {
namespace {

constexpr int AD_CHUNK = 1024;   // elements per workgroup (256 threads x float4)

struct AdamSeg {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;            // 0: parameter without a gradient this step -> untouched (torch skips it too)
  float step_size;      // lr / (1 - beta1^t), t = number of updates of THIS parameter (torch counts per parameter)
  float inv_sqrt_bc2;   // 1 / sqrt(1 - beta2^t)
  float g_clamp;        // > 0: the gradient is clamped to [-g_clamp, g_clamp] first AND written back (the reference's
                        //      `p.grad.data.clamp_(-1, 1)` over the ECC parameters, train_scannetv2.py:247-249, without
                        //      its 20 small launches in front of the optimizer)
  int32_t group;        // row of the group table: the *_groups entry points read it, the one-group ones never do
};

// decay = 1 - lr * weight_decay, omb1 = 1 - beta1, omb2 = 1 - beta2: formed in double on the host and rounded once,
// as torch does (1.0f - 0.999f is off by 5e-5 relative)
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float decay, float omb1, float b2,
                                         float eps, float omb2, float step_size, float inv_sqrt_bc2) {
  p = p * decay;
  m = m + (g - m) * omb1;                        // lerp form, as torch
  v = b2 * v + omb2 * (g * g);
  const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
  p = p - step_size * (m / denom);
}

// p.grad.data.clamp_(-gc, gc) of train_scannetv2.py:246-248: torch's clamp propagates NaN (fminf / fmaxf would
// return the bound and hide a diverged branch)
__device__ __forceinline__ float clamp_keep_nan(float g, float gc) { return g != g ? g : fminf(fmaxf(g, -gc), gc); }

__global__ __launch_bounds__(256) void adamw_kernel(const AdamSeg* __restrict__ segs,
                                                    const int32_t* __restrict__ blocks, float lr, float b1, float b2,
                                                    float eps, float wd) {   // lr = decay, b1 = 1-beta1, wd = 1-beta2
  const int s = blocks[2 * blockIdx.x], chunk = blocks[2 * blockIdx.x + 1];
  const AdamSeg sg = segs[s];
  const float step_size = sg.step_size, inv_sqrt_bc2 = sg.inv_sqrt_bc2;
  const float gc = sg.g_clamp;
  float* const gw = const_cast<float*>(sg.g);
  const int64_t i0 = (int64_t)chunk * AD_CHUNK + (int64_t)threadIdx.x * 4;
  if (i0 >= sg.n) return;
  const bool vec = i0 + 4 <= sg.n && ((reinterpret_cast<uintptr_t>(sg.p + i0) | reinterpret_cast<uintptr_t>(sg.g + i0) |
                                       reinterpret_cast<uintptr_t>(sg.m + i0) | reinterpret_cast<uintptr_t>(sg.v + i0)) & 15) == 0;
  if (vec) {
    float4 p = *reinterpret_cast<float4*>(sg.p + i0);
    float4 g = *reinterpret_cast<const float4*>(sg.g + i0);
    if (gc > 0.0f) {
      g.x = clamp_keep_nan(g.x, gc);
      g.y = clamp_keep_nan(g.y, gc);
      g.z = clamp_keep_nan(g.z, gc);
      g.w = clamp_keep_nan(g.w, gc);
      *reinterpret_cast<float4*>(gw + i0) = g;
    }
    float4 m = *reinterpret_cast<float4*>(sg.m + i0);
    float4 v = *reinterpret_cast<float4*>(sg.v + i0);
    adam_one(p.x, g.x, m.x, v.x, lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2);
    adam_one(p.y, g.y, m.y, v.y, lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2);
    adam_one(p.z, g.z, m.z, v.z, lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2);
    adam_one(p.w, g.w, m.w, v.w, lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2);
    *reinterpret_cast<float4*>(sg.p + i0) = p;
    *reinterpret_cast<float4*>(sg.m + i0) = m;
    *reinterpret_cast<float4*>(sg.v + i0) = v;
  } else {
    for (int64_t i = i0; i < i0 + 4 && i < sg.n; ++i) {
      float p = sg.p[i], m = sg.m[i], v = sg.v[i];
      float g = sg.g[i];
      if (gc > 0.0f) {
        g = clamp_keep_nan(g, gc);
        gw[i] = g;
      }
      adam_one(p, g, m, v, lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2);
      sg.p[i] = p;
      sg.m[i] = m;
      sg.v[i] = v;
    }
  }
}

// ---- dynamic loss scaling for fp16 training (torch.amp.GradScaler: unscale_ + found_inf.item() + step + update, a dozen
// foreach launches and one device->host read per step) in three launches without a read-back.  The state -- scale, overflow
// flag, skip counters -- lives on the device; the host never learns whether a step was skipped.

// the segment as wsis_adamw_step_scaled reads it: the slot of (step_size, inv_sqrt_bc2) carries the HOST's update count
struct AdamSegScaled {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  int64_t t_host;       // updates of this parameter the host has issued, this one included (skipped ones too)
  float g_clamp;
  int32_t group;
};
static_assert(sizeof(AdamSegScaled) == sizeof(AdamSeg) && offsetof(AdamSegScaled, t_host) == offsetof(AdamSeg, step_size) &&
                  offsetof(AdamSegScaled, g_clamp) == offsetof(AdamSeg, g_clamp) && offsetof(AdamSegScaled, n) == offsetof(AdamSeg, n) &&
                  offsetof(AdamSegScaled, group) == offsetof(AdamSeg, group),
              "one table layout for the five entry points");

// inf or NaN: all exponent bits set.  On the bits, so that no floating-point flag can fold the test away.
__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// Reads g only (4 bytes per parameter).  A wave that saw a non-finite element stores 1.0f from one lane: every writer
// stores the same value, nobody reads the flag in this launch, and nothing here ever stores 0.
__global__ __launch_bounds__(256) void grad_nonfinite_kernel(const AdamSeg* __restrict__ segs,
                                                             const int32_t* __restrict__ blocks,
                                                             float* __restrict__ found_inf) {
  const int s = blocks[2 * blockIdx.x], chunk = blocks[2 * blockIdx.x + 1];
  const float* const g = segs[s].g;
  const int64_t n = segs[s].n;
  const int64_t i0 = (int64_t)chunk * AD_CHUNK + (int64_t)threadIdx.x * 4;
  bool bad = false;
  if (i0 < n) {
    if (i0 + 4 <= n && (reinterpret_cast<uintptr_t>(g + i0) & 15) == 0) {
      const float4 x = *reinterpret_cast<const float4*>(g + i0);
      bad = ((int)nonfinite(x.x) | (int)nonfinite(x.y) | (int)nonfinite(x.z) | (int)nonfinite(x.w)) != 0;
    } else {
      for (int64_t i = i0; i < i0 + 4 && i < n; ++i) bad = bad || nonfinite(g[i]);
    }
  }
  const unsigned long long m = __ballot(bad);
  if (m != 0ull && (threadIdx.x & 63) == 0) *found_inf = 1.0f;
}

// The skip counters are race-free by construction: skipped[s] is WRITTEN only in a launch whose flag is set, by one thread
// (thread 0 of chunk 0 of segment s), and in such a launch every other thread returns before it would read a counter; it
// is READ only in a launch whose flag is clear, in which nobody writes it.  The flag itself is read-only here.
__global__ __launch_bounds__(256) void adamw_scaled_kernel(const AdamSegScaled* __restrict__ segs,
                                                           const int32_t* __restrict__ blocks, float decay, float omb1,
                                                           float b2, float eps, float omb2, double lr, double beta1,
                                                           double beta2, const float* __restrict__ grad_scale,
                                                           const float* __restrict__ found_inf,
                                                           int32_t* __restrict__ skipped) {
  __shared__ float corr[3];
  const int s = blocks[2 * blockIdx.x], chunk = blocks[2 * blockIdx.x + 1];
  const AdamSegScaled sg = segs[s];
  if (found_inf && *found_inf != 0.0f) {       // uniform over the launch: nothing of p, m, v or g is written
    if (chunk == 0 && threadIdx.x == 0 && sg.n > 0) skipped[s] += 1;
    return;
  }
  if (threadIdx.x == 0) {
    // updates that took effect; both corrections in double and rounded once, as FlatAdamW.step does on the host
    int64_t t = sg.t_host - (int64_t)skipped[s];
    if (t < 1) t = 1;
    corr[0] = (float)(lr / (1.0 - pow(beta1, (double)t)));
    corr[1] = (float)(1.0 / sqrt(1.0 - pow(beta2, (double)t)));
    corr[2] = grad_scale ? (float)(1.0 / (double)*grad_scale) : 1.0f;      // torch's unscale_ rounding
  }
  __syncthreads();
  const float step_size = corr[0], inv_sqrt_bc2 = corr[1], inv = corr[2];
  const float gc = sg.g_clamp;
  float* const gw = const_cast<float*>(sg.g);
  const int64_t i0 = (int64_t)chunk * AD_CHUNK + (int64_t)threadIdx.x * 4;
  if (i0 >= sg.n) return;
  const bool vec = i0 + 4 <= sg.n && ((reinterpret_cast<uintptr_t>(sg.p + i0) | reinterpret_cast<uintptr_t>(sg.g + i0) |
                                       reinterpret_cast<uintptr_t>(sg.m + i0) | reinterpret_cast<uintptr_t>(sg.v + i0)) & 15) == 0;
  if (vec) {
    float4 p = *reinterpret_cast<float4*>(sg.p + i0);
    float4 g = *reinterpret_cast<const float4*>(sg.g + i0);
    g.x *= inv;
    g.y *= inv;
    g.z *= inv;
    g.w *= inv;
    if (gc > 0.0f) {                           // the clamp acts on the UNSCALED gradient, which is what .grad then holds
      g.x = clamp_keep_nan(g.x, gc);
      g.y = clamp_keep_nan(g.y, gc);
      g.z = clamp_keep_nan(g.z, gc);
      g.w = clamp_keep_nan(g.w, gc);
      *reinterpret_cast<float4*>(gw + i0) = g;
    }
    float4 m = *reinterpret_cast<float4*>(sg.m + i0);
    float4 v = *reinterpret_cast<float4*>(sg.v + i0);
    adam_one(p.x, g.x, m.x, v.x, decay, omb1, b2, eps, omb2, step_size, inv_sqrt_bc2);
    adam_one(p.y, g.y, m.y, v.y, decay, omb1, b2, eps, omb2, step_size, inv_sqrt_bc2);
    adam_one(p.z, g.z, m.z, v.z, decay, omb1, b2, eps, omb2, step_size, inv_sqrt_bc2);
    adam_one(p.w, g.w, m.w, v.w, decay, omb1, b2, eps, omb2, step_size, inv_sqrt_bc2);
    *reinterpret_cast<float4*>(sg.p + i0) = p;
    *reinterpret_cast<float4*>(sg.m + i0) = m;
    *reinterpret_cast<float4*>(sg.v + i0) = v;
  } else {
    for (int64_t i = i0; i < i0 + 4 && i < sg.n; ++i) {
      float p = sg.p[i], m = sg.m[i], v = sg.v[i];
      float g = sg.g[i] * inv;
      if (gc > 0.0f) {
        g = clamp_keep_nan(g, gc);
        gw[i] = g;
      }
      adam_one(p, g, m, v, decay, omb1, b2, eps, omb2, step_size, inv_sqrt_bc2);
      sg.p[i] = p;
      sg.m[i] = m;
      sg.v[i] = v;
    }
  }
}

// ---- several parameter groups in the step's one launch (torch.optim.AdamW with more than one entry in param_groups:
// no weight decay on norm parameters and biases, a lower learning rate for the pre-trained UNet).  The two kernels above
// keep their code; these two take what those get as launch arguments from the row of the group table that the segment
// names in `group`, and share one body.

// one parameter group as the host holds it (param_groups[k] of a torch.optim.AdamW with several groups): a row of the
// group table of the *_groups entry points, in double so that the kernel rounds where the host rounds for one group
struct AdamGroup {
  double lr, beta1, beta2, eps, weight_decay;
};
static_assert(sizeof(AdamGroup) == 40, "wsis_adamw_group_bytes");

// the five constants adam_one takes, each formed in double and rounded once: by the one-group entry points on the host
// (their launch arguments), by the *_groups kernels per workgroup from the segment's group row -- the same expression
struct AdamHyper {
  float decay, omb1, b2, eps, omb2;
};
__host__ __device__ __forceinline__ AdamHyper adam_hyper(double lr, double beta1, double beta2, double eps,
                                                         double weight_decay) {
  return {(float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)eps, (float)(1.0 - beta2)};
}

// One thread's four elements of chunk `chunk` of a segment, as adamw_kernel (SCALED: as adamw_scaled_kernel, the
// gradient multiplied by `inv` before the clamp) walks them: float4 where the four addresses allow it, else element by
// element (the tail of a segment, a gradient view off a 16-byte boundary).  `hyper()` gives the constants and is
// called behind the loads: the group row is one more dependent scalar load, which then waits beside p, g, m, v
// instead of in front of them.
template <bool SCALED, class Hyper>
__device__ __forceinline__ void adam_chunk(float* sp, const float* sg, float* sm, float* sv, int64_t n, float gc, int chunk,
                                           float inv, Hyper hyper, float step_size, float inv_sqrt_bc2) {
  float* const gw = const_cast<float*>(sg);
  const int64_t i0 = (int64_t)chunk * AD_CHUNK + (int64_t)threadIdx.x * 4;
  if (i0 >= n) return;
  const bool vec = i0 + 4 <= n && ((reinterpret_cast<uintptr_t>(sp + i0) | reinterpret_cast<uintptr_t>(sg + i0) |
                                    reinterpret_cast<uintptr_t>(sm + i0) | reinterpret_cast<uintptr_t>(sv + i0)) & 15) == 0;
  if (vec) {
    float4 p = *reinterpret_cast<float4*>(sp + i0);
    float4 g = *reinterpret_cast<const float4*>(sg + i0);
    if (SCALED) {
      g.x *= inv;
      g.y *= inv;
      g.z *= inv;
      g.w *= inv;
    }
    if (gc > 0.0f) {
      g.x = clamp_keep_nan(g.x, gc);
      g.y = clamp_keep_nan(g.y, gc);
      g.z = clamp_keep_nan(g.z, gc);
      g.w = clamp_keep_nan(g.w, gc);
      *reinterpret_cast<float4*>(gw + i0) = g;
    }
    float4 m = *reinterpret_cast<float4*>(sm + i0);
    float4 v = *reinterpret_cast<float4*>(sv + i0);
    const AdamHyper h = hyper();
    adam_one(p.x, g.x, m.x, v.x, h.decay, h.omb1, h.b2, h.eps, h.omb2, step_size, inv_sqrt_bc2);
    adam_one(p.y, g.y, m.y, v.y, h.decay, h.omb1, h.b2, h.eps, h.omb2, step_size, inv_sqrt_bc2);
    adam_one(p.z, g.z, m.z, v.z, h.decay, h.omb1, h.b2, h.eps, h.omb2, step_size, inv_sqrt_bc2);
    adam_one(p.w, g.w, m.w, v.w, h.decay, h.omb1, h.b2, h.eps, h.omb2, step_size, inv_sqrt_bc2);
    *reinterpret_cast<float4*>(sp + i0) = p;
    *reinterpret_cast<float4*>(sm + i0) = m;
    *reinterpret_cast<float4*>(sv + i0) = v;
  } else {
    const AdamHyper h = hyper();
    for (int64_t i = i0; i < i0 + 4 && i < n; ++i) {
      float p = sp[i], m = sm[i], v = sv[i];
      float g = SCALED ? sg[i] * inv : sg[i];
      if (gc > 0.0f) {
        g = clamp_keep_nan(g, gc);
        gw[i] = g;
      }
      adam_one(p, g, m, v, h.decay, h.omb1, h.b2, h.eps, h.omb2, step_size, inv_sqrt_bc2);
      sp[i] = p;
      sm[i] = m;
      sv[i] = v;
    }
  }
}

// wsis_adamw_step_groups: as adamw_kernel, the constants from the segment's group row.  The row's address is uniform
// over the workgroup (five scalar loads, L2-resident after the first workgroup) and every thread converts it itself:
// four fp64 operations and five conversions per wave, no LDS and no barrier.  Measured +5.6 us on the 62 us step of
// the 11.1 M parameter model; the scaled kernel below, where thread 0 converts, costs nothing.
__global__ __launch_bounds__(256) void adamw_groups_kernel(const AdamSeg* __restrict__ segs,
                                                           const int32_t* __restrict__ blocks,
                                                           const AdamGroup* __restrict__ groups) {
  const int s = blocks[2 * blockIdx.x], chunk = blocks[2 * blockIdx.x + 1];
  const AdamSeg sg = segs[s];
  const AdamGroup* const gr = groups + sg.group;
  adam_chunk<false>(sg.p, sg.g, sg.m, sg.v, sg.n, sg.g_clamp, chunk, 1.0f,
                    [gr] { return adam_hyper(gr->lr, gr->beta1, gr->beta2, gr->eps, gr->weight_decay); }, sg.step_size,
                    sg.inv_sqrt_bc2);
}

// wsis_adamw_step_scaled_groups: as adamw_scaled_kernel, with lr, beta1, beta2 of the corrections and the constants of
// the rule from the segment's group row.  Thread 0 reads the row and converts beside its two pow; the five floats ride
// through LDS behind the barrier the corrections need anyway.
__global__ __launch_bounds__(256) void adamw_scaled_groups_kernel(const AdamSegScaled* __restrict__ segs,
                                                                  const int32_t* __restrict__ blocks,
                                                                  const AdamGroup* __restrict__ groups,
                                                                  const float* __restrict__ grad_scale,
                                                                  const float* __restrict__ found_inf,
                                                                  int32_t* __restrict__ skipped) {
  __shared__ float corr[3];
  __shared__ AdamHyper hyper;
  const int s = blocks[2 * blockIdx.x], chunk = blocks[2 * blockIdx.x + 1];
  const AdamSegScaled sg = segs[s];
  if (found_inf && *found_inf != 0.0f) {       // uniform over the launch: every group skips, nothing is written
    if (chunk == 0 && threadIdx.x == 0 && sg.n > 0) skipped[s] += 1;
    return;
  }
  if (threadIdx.x == 0) {
    const AdamGroup gr = groups[sg.group];
    int64_t t = sg.t_host - (int64_t)skipped[s];
    if (t < 1) t = 1;
    corr[0] = (float)(gr.lr / (1.0 - pow(gr.beta1, (double)t)));
    corr[1] = (float)(1.0 / sqrt(1.0 - pow(gr.beta2, (double)t)));
    corr[2] = grad_scale ? (float)(1.0 / (double)*grad_scale) : 1.0f;
    hyper = adam_hyper(gr.lr, gr.beta1, gr.beta2, gr.eps, gr.weight_decay);
  }
  __syncthreads();
  adam_chunk<true>(sg.p, sg.g, sg.m, sg.v, sg.n, sg.g_clamp, chunk, corr[2], [] { return hyper; }, corr[0], corr[1]);
}

// torch._amp_update_scale_ in one thread, then the flag is cleared for the next step
__global__ void loss_scale_update_kernel(float* __restrict__ scale, int32_t* __restrict__ tracker,
                                         float* __restrict__ found_inf, double growth, double backoff, int32_t interval) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (*found_inf != 0.0f) {
    *scale = (float)((double)*scale * backoff);
    *tracker = 0;
  } else {
    const int32_t ok = *tracker + 1;
    if (ok == interval) {
      const float grown = (float)((double)*scale * growth);
      if (!nonfinite(grown)) *scale = grown;
      *tracker = 0;
    } else {
      *tracker = ok;
    }
  }
  *found_inf = 0.0f;
}

}  // namespace
}  // namespace wsis

using namespace wsis;

extern "C" {

int32_t wsis_adamw_segment_bytes(void) { return (int32_t)sizeof(AdamSeg); }
int32_t wsis_adamw_group_bytes(void) { return (int32_t)sizeof(AdamGroup); }
int32_t wsis_adamw_chunk(void) { return AD_CHUNK; }

int wsis_adamw_step(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks, double lr, double beta1,
                    double beta2, double eps, double weight_decay, void* stream) {
  WSIS_REQUIRE(n_blocks >= 0, "bad args");
  if (n_blocks == 0) return WSIS_OK;
  WSIS_REQUIRE(d_segments && d_blocks, "null pointer");
  WSIS_REQUIRE(n_blocks < ((int64_t)1 << 31), "too many blocks");
  const AdamHyper h = adam_hyper(lr, beta1, beta2, eps, weight_decay);
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)n_blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const AdamSeg*>(d_segments), d_blocks, h.decay, h.omb1, h.b2, h.eps, h.omb2);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_adamw_step_groups(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks, const void* d_groups,
                           int32_t n_groups, void* stream) {
  WSIS_REQUIRE(n_blocks >= 0 && n_groups >= 1, "bad args");
  if (n_blocks == 0) return WSIS_OK;
  WSIS_REQUIRE(d_segments && d_blocks && d_groups, "null pointer");
  WSIS_REQUIRE(n_blocks < ((int64_t)1 << 31), "too many blocks");
  hipLaunchKernelGGL(adamw_groups_kernel, dim3((unsigned)n_blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const AdamSeg*>(d_segments), d_blocks, static_cast<const AdamGroup*>(d_groups));
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_grad_nonfinite(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks, float* d_found_inf,
                        void* stream) {
  WSIS_REQUIRE(n_blocks >= 0, "bad args");
  if (n_blocks == 0) return WSIS_OK;
  WSIS_REQUIRE(d_segments && d_blocks && d_found_inf, "null pointer");
  WSIS_REQUIRE(n_blocks < ((int64_t)1 << 31), "too many blocks");
  hipLaunchKernelGGL(grad_nonfinite_kernel, dim3((unsigned)n_blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const AdamSeg*>(d_segments), d_blocks, d_found_inf);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_adamw_step_scaled(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks, double lr, double beta1,
                           double beta2, double eps, double weight_decay, const float* d_grad_scale,
                           const float* d_found_inf, int32_t* d_skipped, void* stream) {
  WSIS_REQUIRE(n_blocks >= 0, "bad args");
  if (n_blocks == 0) return WSIS_OK;
  WSIS_REQUIRE(d_segments && d_blocks, "null pointer");
  WSIS_REQUIRE(d_skipped, "null skip counters");
  WSIS_REQUIRE(n_blocks < ((int64_t)1 << 31), "too many blocks");
  const AdamHyper h = adam_hyper(lr, beta1, beta2, eps, weight_decay);
  hipLaunchKernelGGL(adamw_scaled_kernel, dim3((unsigned)n_blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const AdamSegScaled*>(d_segments), d_blocks, h.decay, h.omb1, h.b2, h.eps, h.omb2, lr,
                     beta1, beta2, d_grad_scale, d_found_inf, d_skipped);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_adamw_step_scaled_groups(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks,
                                  const void* d_groups, int32_t n_groups, const float* d_grad_scale,
                                  const float* d_found_inf, int32_t* d_skipped, void* stream) {
  WSIS_REQUIRE(n_blocks >= 0 && n_groups >= 1, "bad args");
  if (n_blocks == 0) return WSIS_OK;
  WSIS_REQUIRE(d_segments && d_blocks && d_groups, "null pointer");
  WSIS_REQUIRE(d_skipped, "null skip counters");
  WSIS_REQUIRE(n_blocks < ((int64_t)1 << 31), "too many blocks");
  hipLaunchKernelGGL(adamw_scaled_groups_kernel, dim3((unsigned)n_blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const AdamSegScaled*>(d_segments), d_blocks, static_cast<const AdamGroup*>(d_groups),
                     d_grad_scale, d_found_inf, d_skipped);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

int wsis_loss_scale_update(float* d_scale, int32_t* d_growth_tracker, float* d_found_inf, double growth_factor,
                           double backoff_factor, int32_t growth_interval, void* stream) {
  WSIS_REQUIRE(d_scale && d_growth_tracker && d_found_inf, "null pointer");
  WSIS_REQUIRE(growth_interval >= 1, "bad args");
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, as_stream(stream), d_scale, d_growth_tracker,
                     d_found_inf, growth_factor, backoff_factor, growth_interval);
  WSIS_LAUNCH_CHECK();
  return WSIS_OK;
}

}  // extern "C"
