// The masks of whole tracks, from what the link left on the device: udet_follow_tracks_ragged turns a choice of rows --
// one 64-bit word per frame, bit r = keep row r -- back into binary masks for n frames (packed layout, sample i = H_i x W_i at offsets[i])
// and counts per frame the kept and the dropped foreground and what the kept pixels share with the annotation.
//   1. follow_init_kernel    zeroes stats and writes every row's rank at its root into the workspace -- the lookup of the link
//                            (track_rows.h): one int32 per pixel, never zeroed, a lookup counts only when the row it names holds that root
//   2. follow_paint_kernel   one lane per pixel, a wave on 64 consecutive pixels of one sample: label, lookup, the row's root from LDS, then
//                            one bit of the frame's keep word -- uniform over the workgroup, so a scalar load and a shift, no table; four
//                            lanes' bytes make one aligned 32-bit word of `selected` (packed_bytes.h); the four counts are ballots summed
//                            per wave, reduced in LDS, then one 64-bit integer atomic per non-zero partial per workgroup
// Two launches whatever n, k, the components and the sequences are; integer atomics only, no workgroup waits for another: identical from
// run to run and for a sample alone or inside a batch.  A label outside 1..H_i*W_i is background and a looked-up rank counts only below
// the frame's rows, so nothing indexes outside its own sample whatever labels, dets, counts, keep and the workspace hold; offsets / hw
// are validated by the host caller (native_follow.follow_tracks).
#include "common.h"
#include "host_checks.h"
#include "packed_bytes.h"
#include "track_rows.h"

namespace udet {

#define FOLLOW_PPT 16  // pixels per thread of the paint grid: 4096 pixels per workgroup, as for the instance maps
#define FOLLOW_K UDET_DET_MAX_K
static_assert(FOLLOW_K <= 64, "a frame's keep set is one 64-bit word");

__global__ __launch_bounds__(256) void follow_init_kernel(int n, const long long* __restrict__ offsets, const int* __restrict__ hw,
                                                          const long long* __restrict__ dets, const long long* __restrict__ counts, int k,
                                                          unsigned long long* __restrict__ stats, int* __restrict__ lookup) {
  const size_t stride = (size_t)gridDim.x * 256, g = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t j = g; j < (size_t)n * k; j += stride) {
    const int i = (int)(j / k), r = (int)(j - (size_t)i * k);
    link_enter_roots(dets + (size_t)i * k * UDET_DET_FIELDS, link_rows(counts + 3 * i, k), (long long)hw[2 * i] * hw[2 * i + 1],
                     lookup + offsets[i], r);
  }
  for (size_t j = g; j < (size_t)4 * n; j += stride) stats[j] = 0;
}

__global__ __launch_bounds__(256) void follow_paint_kernel(const int* __restrict__ labels, const long long* __restrict__ offsets,
                                                           const int* __restrict__ hw, const long long* __restrict__ dets,
                                                           const long long* __restrict__ counts, int k,
                                                           const unsigned long long* __restrict__ keep, const unsigned char* __restrict__ gt,
                                                           const int* __restrict__ lookup, unsigned char* __restrict__ selected,
                                                           unsigned long long* __restrict__ stats) {
  __shared__ int root_s[FOLLOW_K], st[4];
  const int i = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const long long HW = (long long)hw[2 * i] * hw[2 * i + 1], off = offsets[i];
  // the sample's pixels are walked from the aligned word its first byte lies in: pixel p sits at position p + a of that walk
  const int a = (int)((reinterpret_cast<uintptr_t>(selected) + (unsigned long long)off) & 3);
  const long long span = HW + a;
  if ((long long)blockIdx.x * 256 >= span) return;  // beyond this sample's pixels (the whole workgroup)
  const int rows = link_rows(counts + 3 * i, k);
  const unsigned long long kw = keep[i];  // uniform over the workgroup; bits at or above rows are never looked at
  for (int j = t; j < k; j += 256) {
    const long long root = j < rows ? dets[((size_t)i * k + j) * UDET_DET_FIELDS] : -1;
    root_s[j] = (root >= 0 && root < HW) ? (int)root : -1;
  }
  if (t < 4) st[t] = 0;
  __syncthreads();
  const int* __restrict__ lab = labels + off;
  const int* __restrict__ look = lookup + off;
  const unsigned char* __restrict__ ann = gt ? gt + off : nullptr;
  unsigned char* __restrict__ out = selected + off;
  int n_kept = 0, n_dropped = 0, n_hit = 0, n_gt = 0;  // of this wave
  for (long long base = (long long)blockIdx.x * 256; base < span; base += (long long)gridDim.x * 256) {  // block-uniform bounds
    const long long p = base + t - a;
    const bool valid = p >= 0 && p < HW;
    const int L = valid ? lab[p] : 0;
    const bool g = valid && ann && ann[p] != 0;
    const bool fg = L >= 1 && L <= HW;
    bool kept = false;
    if (fg) {
      const int c = look[L - 1];  // never zeroed: only a rank whose row holds this root counts
      kept = (unsigned)c < (unsigned)rows && root_s[c] == L - 1 && ((kw >> c) & 1ull);
    }
    n_kept += __popcll(__ballot(kept));
    n_dropped += __popcll(__ballot(fg && !kept));
    n_hit += __popcll(__ballot(kept && g));
    n_gt += __popcll(__ballot(g));
    store_packed_byte(out, p, HW, lane, valid, kept ? 1u : 0u);
  }
  if (lane == 0) {  // a workgroup sees fewer than 2^31 pixels
    if (n_kept) atomicAdd(st + 0, n_kept);
    if (n_dropped) atomicAdd(st + 1, n_dropped);
    if (n_hit) atomicAdd(st + 2, n_hit);
    if (n_gt) atomicAdd(st + 3, n_gt);
  }
  __syncthreads();
  if (t < 4 && st[t]) atomicAdd(stats + (size_t)4 * i + t, (unsigned long long)st[t]);
}

}  // namespace udet

using namespace udet;

extern "C" {

size_t udet_follow_tracks_workspace_bytes(size_t total_pixels, int n, int k) {
  if (n < 1 || n > 65535 || total_pixels < 1 || k < 1 || k > UDET_DET_MAX_K) return 0;
  return total_pixels * sizeof(int);  // the root-to-rank lookup; no per-sample term
}

int udet_follow_tracks_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                              long long total_pixels, const long long* dets, const long long* counts, int k,
                              const unsigned long long* keep, const unsigned char* gt, unsigned char* selected, long long* stats,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch("follow_tracks_ragged", n, max_h, max_w, total_pixels < 0 ? 0 : (size_t)total_pixels)) return UDET_ERR_ARG;
  if (!labels || !offsets || !hw || !dets || !counts || !keep || !selected || !stats) {
    set_error("follow_tracks_ragged: bad argument (non-null labels, offsets, hw, dets, counts, keep, selected and stats)");
    return UDET_ERR_ARG;
  }
  if (k < 1 || k > UDET_DET_MAX_K) {
    set_error("follow_tracks_ragged: k = %d in 1..UDET_DET_MAX_K = %d is required", k, UDET_DET_MAX_K);
    return UDET_ERR_ARG;
  }
  if (bad_workspace("follow_tracks_ragged", workspace, workspace_bytes, udet_follow_tracks_workspace_bytes((size_t)total_pixels, n, k), 4))
    return UDET_ERR_ARG;
  const uintptr_t a8 = reinterpret_cast<uintptr_t>(dets) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(keep) |
                       reinterpret_cast<uintptr_t>(stats);
  if ((reinterpret_cast<uintptr_t>(labels) & 3) || (a8 & 7)) {
    set_error("follow_tracks_ragged: labels must be 4-byte aligned, dets, counts, keep and stats 8-byte aligned");
    return UDET_ERR_ARG;
  }
  const long nb = ((long)max_h * max_w + 3 + 256 * FOLLOW_PPT - 1) / (256 * FOLLOW_PPT);  // + 3: the walk starts at an aligned word
  const size_t nz = ((size_t)n * k + 255) / 256;  // >= ceil(4 n / 256) as well: the loops stride over both
  int* lookup = (int*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(follow_init_kernel, dim3((unsigned)(nz > 65536 ? 65536 : nz)), dim3(256), 0, s, n, offsets, hw, dets, counts, k,
                     (unsigned long long*)stats, lookup);
  hipLaunchKernelGGL(follow_paint_kernel, dim3((unsigned)nb, n), dim3(256), 0, s, labels, offsets, hw, dets, counts, k, keep, gt, lookup,
                     selected, (unsigned long long*)stats);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // extern "C"
