// The sequence stage of the post-processing pass, batched:
//   udet_post_propagate_sequences   generate_soft_score_from_buffer.py propagate :127-231 for many sequences and both directions in two
//                                   launches, given the flows -- what post_processing.propagate does with four launches per frame and
//                                   direction (udet_post_remap x 2, udet_post_blend x 2), bit for bit
//   udet_post_select_unary          crf_refine.py:40-52 (candidate choice) and :113-121 (unary energies, identity Gaussian) for a batch of
//                                   same-size frames in two launches, laid out as udet_dense_crf_ragged reads them
// The per-pixel expressions of the propagation are those of postproc.hip (post_remap.h).  Compiled with -ffp-contract=off (Makefile).
#include <math.h>

#include "common.h"
#include "host_checks.h"
#include "post_remap.h"

namespace udet {

// partial maxima of one (frame, direction) in the workspace: the maxima launch cuts a frame into this many interleaved slices
constexpr int kMaxParts = 32;

// max over a workgroup of 1024 threads (16 waves): shuffles inside a wave, one LDS word per wave.  max is exact in any order.  `sm` must
// not be read or written by another reduction until the workgroup has passed a later barrier.
__device__ __forceinline__ float block_max_1024(float v, float* sm) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sm[0];
  for (int k = 1; k < 16; ++k) r = fmaxf(r, sm[k]);
  return r;
}

// remap(src, flow)(i) of a frame W wide; a pixel's (u, v) is one 8-byte load
__device__ __forceinline__ float remap_pixel(const float* __restrict__ src, const float* __restrict__ fl, unsigned i, int H, int W) {
  const unsigned y = i / (unsigned)W, x = i - y * W;
  const float2 uv = reinterpret_cast<const float2*>(fl)[i];
  return remap_gather(src, remap_taps(uv.x, uv.y, x, y), H, W);
}

// direction 0 (forward pass): frame k pulls from k - 1 along flow_prev[k]; direction 1 (backward pass): from k + 1 along flow_next[k]
struct SeqArgs {
  const float* masks;
  const float* flow[2];
  const int* seq_first;
  const int* seq_len;
  float* avg[2];
  float* part;  // [2][total][kMaxParts]
  int total, H, W;
  float a, b;   // the weights of the pulled mask and of the pulled running average
};

// (a) max(remap(mask[k -+ 1], flow[k])) of every step: independent of the recurrence.  Workgroup (slice, sequence, direction) walks the
// steps of its sequence and writes the maximum over its slice of the pixels (pixels slice * 256 + t, stride kMaxParts * 256); the chain
// launch takes the maximum of the kMaxParts slices.  No atomics.
__global__ __launch_bounds__(256) void seq_maxima_kernel(SeqArgs a) {
  __shared__ float sm[4];
  const int dir = blockIdx.z, first = a.seq_first[blockIdx.y], len = a.seq_len[blockIdx.y];
  const unsigned hw = (unsigned)a.H * a.W, t = threadIdx.x;  // h * w < 2^31: i + stride cannot wrap
  for (int j = 1; j < len; ++j) {
    const int k = dir ? first + len - 1 - j : first + j, from = dir ? k + 1 : k - 1;
    const float* __restrict__ src = a.masks + (size_t)from * hw;
    const float* __restrict__ fl = a.flow[dir] + (size_t)k * hw * 2;
    float mx = -INFINITY;
    for (unsigned i = blockIdx.x * 256 + t; i < hw; i += kMaxParts * 256) mx = fmaxf(mx, remap_pixel(src, fl, i, a.H, a.W));
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((t & 63) == 0) sm[t >> 6] = mx;
    __syncthreads();
    if (t == 0) a.part[((size_t)dir * a.total + k) * kMaxParts + blockIdx.x] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    __syncthreads();
  }
}

// (b) the recurrence: one workgroup per (sequence, direction) walks the frames.  avg[k] is the state: a step gathers avg[k -+ 1], which
// the same workgroup finished before the barrier that ends the step before (workgroup scope: one CU, one L1).  Per step and pixel,
// thread t owns pixels t, t + 1024, ...:
//   pass 1  ra_w = remap(avg[k -+ 1], flow[k]) -> avg[k] (its own slot, re-read by the same thread), block max
//   pass 2  r = a * (remap(mask[k -+ 1], flow[k]) / den(max from launch (a))) + b * (ra_w / den(max ra_w)) -> avg[k], block max
//   pass 3  avg[k] = r / den(max r)
// post_blend_kernel's first call (a = 1, b = 0) is 1.f * v = v exactly.
__global__ __launch_bounds__(1024) void seq_chain_kernel(SeqArgs a) {
  __shared__ float sm_a[16], sm_b[16];
  const int dir = blockIdx.y, first = a.seq_first[blockIdx.x], len = a.seq_len[blockIdx.x];
  const unsigned hw = (unsigned)a.H * a.W, t = threadIdx.x;  // h * w < 2^31: i + stride cannot wrap
  float* avg = a.avg[dir];
  {
    const int k0 = dir ? first + len - 1 : first;
    const float* m = a.masks + (size_t)k0 * hw;
    float* out = avg + (size_t)k0 * hw;
    for (unsigned i = t; i < hw; i += 1024) out[i] = m[i];
  }
  __syncthreads();
  for (int j = 1; j < len; ++j) {
    const int k = dir ? first + len - 1 - j : first + j, from = dir ? k + 1 : k - 1;
    const float* __restrict__ prev_avg = avg + (size_t)from * hw;
    const float* __restrict__ prev_mask = a.masks + (size_t)from * hw;
    const float* __restrict__ fl = a.flow[dir] + (size_t)k * hw * 2;
    float* __restrict__ out = avg + (size_t)k * hw;  // frame k: nothing a step reads through the other pointers
    float mx = -INFINITY;
    for (unsigned i = t; i < hw; i += 1024) {
      const float v = remap_pixel(prev_avg, fl, i, a.H, a.W);
      out[i] = v;
      mx = fmaxf(mx, v);
    }
    const float den_ra = max_denominator(block_max_1024(mx, sm_a));
    const float* part = a.part + ((size_t)dir * a.total + k) * kMaxParts;
    float ms = part[0];
    for (int p = 1; p < kMaxParts; ++p) ms = fmaxf(ms, part[p]);
    const float den_s = max_denominator(ms);
    float my = -INFINITY;
    for (unsigned i = t; i < hw; i += 1024) {
      const float s2 = remap_pixel(prev_mask, fl, i, a.H, a.W);
      const float ra = out[i] / den_ra;
      const float r = blend_pair(a.a, s2 / den_s, a.b, ra);
      out[i] = r;
      my = fmaxf(my, r);
    }
    const float den2 = max_denominator(block_max_1024(my, sm_b));
    for (unsigned i = t; i < hw; i += 1024) out[i] = out[i] / den2;
    __syncthreads();  // avg[k] is complete and visible to the workgroup before the next step gathers from it
  }
}

// ---- candidate choice and unary ----------------------------------------------------------------------------------------------------
template <typename T, typename Op>
__device__ __forceinline__ T tree_reduce_1024(T v, T* sm, Op op) {  // a fixed order: the result does not depend on timing
  const int t = threadIdx.x;
  sm[t] = v;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (t < s) sm[t] = op(sm[t], sm[t + s]);
    __syncthreads();
  }
  const T r = sm[0];
  __syncthreads();
  return r;
}

// launch 1, workgroup (frame, candidate): score = sum(p * gt) / (sum(p) + 1e-8) (crf_refine.py:40-43; the product in float32 like
// np.multiply, the sums in double, a fixed order) -> scores[frame][candidate]
__global__ __launch_bounds__(1024) void select_stats_kernel(const float* __restrict__ pred, const float* __restrict__ avg_f,
                                                            const float* __restrict__ avg_b, const float* __restrict__ gt, int hw,
                                                            double* __restrict__ scores) {
  __shared__ double sm[1024];
  const int f = blockIdx.x, c = blockIdx.y;
  const float* p = (c == 0 ? pred : (c == 1 ? avg_f : avg_b)) + (size_t)f * hw;
  const float* g = gt + (size_t)f * hw;
  double spg = 0.0, sp = 0.0;
  for (int i = threadIdx.x; i < hw; i += 1024) {
    const float v = p[i];
    spg += (double)(v * g[i]);
    sp += (double)v;
  }
  auto add = [](double x, double y) { return x + y; };
  spg = tree_reduce_1024(spg, sm, add);
  sp = tree_reduce_1024(sp, sm, add);
  if (threadIdx.x == 0) scores[f * 3 + c] = spg / (sp + 1e-8);
}

// launch 2, one workgroup per frame: the reference's rule on (m, f, b) = scores[frame], the chosen candidate copied to soft, its maximum
// (exact in any order) and its unary: U = clamp(p / (max + 1e-8), 1e-6, 1 - 1e-6) in double, -log(1 - U) -> unary[0], -log(U) -> unary[1], sample i at i * hw
__global__ __launch_bounds__(1024) void select_unary_kernel(const float* __restrict__ pred, const float* __restrict__ avg_f,
                                                            const float* __restrict__ avg_b, int n, int hw,
                                                            const double* __restrict__ scores, int* __restrict__ choice, float* __restrict__ soft, float* __restrict__ unary) {
  __shared__ float sm[16];
  const int f = blockIdx.x;
  const double m = scores[f * 3], sf = scores[f * 3 + 1], sb = scores[f * 3 + 2];
  const int c = (m >= sf && m >= sb) ? 0 : ((sf >= m && sf >= sb) ? 1 : 2);
  if (threadIdx.x == 0) choice[f] = c;
  const float* p = (c == 0 ? pred : (c == 1 ? avg_f : avg_b)) + (size_t)f * hw;
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < hw; i += 1024) mx = fmaxf(mx, p[i]);
  const double den = (double)block_max_1024(mx, sm) + 1e-8;
  float* so = soft + (size_t)f * hw;
  float* u0 = unary + (size_t)f * hw;
  float* u1 = unary + (size_t)n * hw + (size_t)f * hw;
  for (int i = threadIdx.x; i < hw; i += 1024) {
    const float v = p[i];
    so[i] = v;
    double U = (double)v / den;
    U = fmin(fmax(U, 1e-6), 1.0 - 1e-6);
    u0[i] = (float)-log(1.0 - U);
    u1[i] = (float)-log(U);
  }
}

}  // namespace udet

using namespace udet;

extern "C" {

size_t udet_post_propagate_workspace_bytes(int total_frames, int n_seq) {
  if (total_frames < 1 || n_seq < 1) return 0;
  return (size_t)total_frames * 2 * kMaxParts * sizeof(float);
}

int udet_post_propagate_sequences(const float* masks, const float* flow_prev, const float* flow_next, int n_seq, const int* seq_first,
                                  const int* seq_len, int total_frames, int h, int w, float w_s, float w_r, float* avg_f, float* avg_b,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch("post_propagate_sequences", n_seq, h, w, total_frames < 1 ? 0 : (size_t)total_frames)) return UDET_ERR_ARG;
  if (!masks || !flow_prev || !flow_next || !seq_first || !seq_len || !avg_f || !avg_b) {
    set_error("post_propagate_sequences: bad argument (non-null masks, flow_prev, flow_next, seq_first, seq_len, avg_f and avg_b)");
    return UDET_ERR_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(flow_prev) | reinterpret_cast<uintptr_t>(flow_next)) & 7) {  // a pixel's (u, v) is one 8-byte load
    set_error("post_propagate_sequences: flow_prev and flow_next must be 8-byte aligned");
    return UDET_ERR_ARG;
  }
  if (avg_f == avg_b || avg_f == masks || avg_b == masks) {
    set_error("post_propagate_sequences: masks, avg_f and avg_b must be three different buffers");
    return UDET_ERR_ARG;
  }
  if (bad_workspace("post_propagate_sequences", workspace, workspace_bytes, udet_post_propagate_workspace_bytes(total_frames, n_seq), 16))
    return UDET_ERR_ARG;
  SeqArgs a;
  a.masks = masks; a.flow[0] = flow_prev; a.flow[1] = flow_next;
  a.seq_first = seq_first; a.seq_len = seq_len;
  a.avg[0] = avg_f; a.avg[1] = avg_b;
  a.part = (float*)workspace;
  a.total = total_frames; a.H = h; a.W = w;
  a.a = w_s; a.b = w_r;
  hipStream_t s = (hipStream_t)stream;
  UDET_LAUNCH(seq_maxima_kernel, dim3(kMaxParts, n_seq, 2), dim3(256), 0, s, a);
  UDET_LAUNCH(seq_chain_kernel, dim3(n_seq, 2), dim3(1024), 0, s, a);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

int udet_post_select_unary(const float* pred, const float* avg_f, const float* avg_b, const float* gt, int n, int hw, int* choice,
                           double* scores, float* soft, float* unary, void* stream) {
  if (n < 1 || n > 65535 || hw < 1 || !pred || !avg_f || !avg_b || !gt || !choice || !scores || !soft || !unary ||
      (reinterpret_cast<uintptr_t>(scores) & 7)) {
    set_error("post_select_unary: bad argument (n = %d in 1..65535, %d pixels per frame, non-null pred, avg_f, avg_b, gt, choice, scores "
              "(8-byte aligned), soft and unary)", n, hw);
    return UDET_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  UDET_LAUNCH(select_stats_kernel, dim3(n, 3), dim3(1024), 0, s, pred, avg_f, avg_b, gt, hw, scores);
  UDET_LAUNCH(select_unary_kernel, dim3(n), dim3(1024), 0, s, pred, avg_f, avg_b, n, hw, (const double*)scores, choice, soft, unary);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // extern "C"
