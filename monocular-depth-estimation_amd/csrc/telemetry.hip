// Step telemetry for the training driver (mdemi/train/loop.py): the parameter
// norm over the optimizer's tensor table and a device-side ring of per-step
// (loss, gradient sum of squares) records, so a train step -- eager or a
// replayed hipGraph -- can be observed without a host synchronisation per step.
// The reference logged the parameter norm (utils/common_utils.py:65-75
// compute_param_norm); its driver (run.py) is absent from the snapshot.
#include <cmath>

#include "common.h"
#include "mdemi_ext.h"

namespace mdemi {

// the optimizer's (tensor, chunk) work items (misc.hip; mdemi_multi_tensor_chunk)
constexpr int TEL_THREADS = 256;
constexpr int TEL_CHUNK = 65536;

// per-(tensor, chunk) sum of squares of the parameters: sumsq_partial's (misc.hip)
// association -- four float4 streams per thread over the 16-B-aligned body, a scalar
// tail, (s0 + s1) + (s2 + s3), then the wave and block sums -- read from t.param
__global__ __launch_bounds__(TEL_THREADS) void param_sumsq_partial(const mdemi_tensor_ref* __restrict__ tl, int nt,
                                                                   const int* __restrict__ chunk_tensor,
                                                                   const int* __restrict__ chunk_index,
                                                                   float* __restrict__ part) {
  __shared__ float red[TEL_THREADS / 64];
  const int item = blockIdx.x;
  const int ti = chunk_tensor[item];
  if (ti < 0 || ti >= nt) {  // a malformed item map contributes nothing (uniform per block)
    if (threadIdx.x == 0) part[item] = 0.f;
    return;
  }
  const mdemi_tensor_ref t = tl[ti];
  const int64_t beg = (int64_t)chunk_index[item] * TEL_CHUNK;
  const int64_t end = min(t.numel, beg + TEL_CHUNK);
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
  const bool vec = ((uintptr_t)t.param & 15) == 0;
  const int64_t vend = vec && end > beg ? beg + ((end - beg) & ~(int64_t)3) : beg;
  constexpr int64_t STEP = 4 * TEL_THREADS;
  int64_t i = beg + 4 * threadIdx.x;
  for (; i + 3 * STEP < vend; i += 4 * STEP) {
    float4 p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) p[u] = *reinterpret_cast<const float4*>(t.param + i + u * STEP);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      s4[u] = fmaf(p[u].x, p[u].x, s4[u]); s4[u] = fmaf(p[u].y, p[u].y, s4[u]);
      s4[u] = fmaf(p[u].z, p[u].z, s4[u]); s4[u] = fmaf(p[u].w, p[u].w, s4[u]);
    }
  }
  for (; i < vend; i += STEP) {
    const float4 p = *reinterpret_cast<const float4*>(t.param + i);
    s4[0] = fmaf(p.x, p.x, s4[0]); s4[0] = fmaf(p.y, p.y, s4[0]);
    s4[0] = fmaf(p.z, p.z, s4[0]); s4[0] = fmaf(p.w, p.w, s4[0]);
  }
  for (int64_t j = vend + threadIdx.x; j < end; j += TEL_THREADS) {
    const float p = t.param[j];
    s4[1] = fmaf(p, p, s4[1]);
  }
  float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  s = block_sum<TEL_THREADS>(s, red);
  if (threadIdx.x == 0) part[item] = s;
}

// fp64 sum of the per-item partials in a fixed order (sumsq_final's, misc.hip)
__global__ __launch_bounds__(256) void param_sumsq_final(const float* __restrict__ part, int nitems,
                                                         float* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nitems; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)red[0];
}

// one thread appends one record; the counters live on the device, so a captured graph
// advances them on every replay
__global__ void telemetry_push_kernel(mdemi_step_record* __restrict__ ring, int capacity,
                                      mdemi_telemetry_state* __restrict__ state, const float* __restrict__ loss,
                                      const float* __restrict__ grad_sumsq) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int32_t n = state->pushed;
  const float l = loss[0];
  const float g = grad_sumsq ? grad_sumsq[0] : -1.f;
  uint32_t flags = 0;
  if (!isfinite(l)) flags |= MDEMI_STEP_LOSS_NONFINITE;
  if (grad_sumsq && !isfinite(g)) flags |= MDEMI_STEP_GRAD_NONFINITE;
  // pushed wraps after 2^31 steps; the slot stays inside the ring either way
  const int slot = (int)((uint32_t)n % (uint32_t)capacity);
  mdemi_step_record r;
  r.loss = l;
  r.grad_sumsq = g;
  r.index = n;
  r.flags = flags;
  ring[slot] = r;
  if (flags) {
    state->nonfinite_steps += 1;
    if (state->first_nonfinite < 0) state->first_nonfinite = n;
  }
  state->pushed = n + 1;
}

}  // namespace mdemi

using namespace mdemi;

extern "C" int mdemi_param_sumsq(const mdemi_tensor_ref* tensors_dev, int32_t ntensors, int64_t nitems, float* sumsq,
                                 void* workspace, void* stream) {
  MDEMI_REQUIRE(tensors_dev && ntensors > 0 && nitems > 0 && nitems <= INT32_MAX && sumsq && workspace,
                "param_sumsq: bad args");
  if (mdemi_multi_tensor_chunk() != TEL_CHUNK) {
    set_error("param_sumsq: chunk size differs from the optimizer's");
    return MDEMI_EINVAL;
  }
  const int* ct = (const int*)workspace;  // mdemi_grad_norm_workspace_size's layout
  const int* ci = ct + nitems;
  float* part = (float*)(ci + nitems);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(param_sumsq_partial, dim3((unsigned)nitems), dim3(TEL_THREADS), 0, st, tensors_dev,
                     (int)ntensors, ct, ci, part);
  hipLaunchKernelGGL(param_sumsq_final, dim3(1), dim3(256), 0, st, part, (int)nitems, sumsq);
  return check_launch("param_sumsq");
}

extern "C" int mdemi_telemetry_push(mdemi_step_record* ring, int32_t capacity, mdemi_telemetry_state* state,
                                    const float* loss, const float* grad_sumsq, void* stream) {
  MDEMI_REQUIRE(ring && capacity > 0 && state && loss, "telemetry_push: bad args");
  hipLaunchKernelGGL(telemetry_push_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ring, (int)capacity, state,
                     loss, grad_sumsq);
  return check_launch("telemetry_push");
}
