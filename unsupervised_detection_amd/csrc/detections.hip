// Every connected component of a ragged batch as a scored box: udet_component_boxes_ragged turns the labels
// components.hip writes (root + 1 on a foreground pixel, 0 on background; packed layout, sample i = H_i x W_i int32 at offsets[i]) into
// the top-k components per sample by area -- root, area, box, centroid numerators, score sum -- and udet_draw_boxes_ragged paints the
// frames of those boxes onto packed rgb frames.  Four launches for the boxes however many samples and components there are:
//   1. det_init_kernel    zeroes the per-pixel area counters and the per-sample counters of the workspace
//   2. det_area_kernel    area per root with one integer atomic per horizontal run of a wave (the root of the wave's first run: one for
//                         the whole wave); the adder whose atomic takes a root's area from below min_area to min_area or above --
//                         exactly one per kept root -- appends the root to the sample's list (the list's order depends on arrival,
//                         nothing read from it does); roots counted per sample
//   3. det_rank_kernel    one workgroup per sample, k rounds over its list: each round takes the best (area, then the smaller root)
//                         candidate strictly worse than the previous winner, a block reduce per round; the winners' rows of `dets` get
//                         root and area and the neutral elements of the box, every other row -1, 0, ...; the winner's area counter is
//                         replaced by -1 - rank; counts
//   4. det_accum_kernel   every pixel of a winner: box, sum_y, sum_x, score sum, one LDS atomic set per horizontal run of a wave into
//                         the workgroup's k x 7 partials, then one 64-bit integer atomicMin / atomicMax / atomicAdd per touched value
//                         straight into `dets`
// Integer work only, no workgroup waits for another: the outputs are exact, identical from run to run and for a sample alone or inside
// a batch.  A label outside 1..H_i*W_i is background, so no label indexes outside its own sample; every other index comes from offsets /
// hw, which the caller validates on the host (native_results.check_component_tables).  Runs are cut where the label changes, so labels
// that are no valid labelling still give each distinct value its own exact sums.
#include "common.h"
#include "elementwise.h"
#include "wave_runs.h"

namespace udet {

#define DET_PPT 8     // pixels per thread of the pixel grids
#define DET_K UDET_DET_MAX_K
#define DET_ACC 7      // accumulated per winner: y0, x0, y1, x1 (min / max), sum_y, sum_x, score_sum (add)
#define DET_NONE 0x7fffffff

static_assert(DET_K <= 64 && UDET_DET_FIELDS == 2 + DET_ACC, "row layout of include/udet.h");

__global__ __launch_bounds__(256) void det_init_kernel(int* __restrict__ area, size_t total_pixels, int* __restrict__ counters, int n) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < total_pixels; k += stride) area[k] = 0;
  if (blockIdx.x == 0)
    for (int j = threadIdx.x; j < 2 * n; j += 256) counters[j] = 0;
}

__global__ __launch_bounds__(256) void det_area_kernel(const int* __restrict__ labels, const long long* __restrict__ offsets,
                                                       const int* __restrict__ hw, int min_area, int* __restrict__ area,
                                                       int* __restrict__ list, int* __restrict__ counters) {
  const int i = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int W = hw[2 * i + 1];
  const long long HW = (long long)hw[2 * i] * W;
  const size_t o = (size_t)offsets[i];
  int roots = 0;
  for (long long base = (long long)blockIdx.x * 256; base < HW; base += (long long)gridDim.x * 256) {  // block-uniform bounds
    const long long k = base + t;
    const bool valid = k < HW;
    const int v = valid ? labels[o + k] : 0;
    const int r = (v >= 1 && v <= HW) ? v - 1 : -1;
    const int x = valid ? (int)k % W : 0;  // HW < 2^31
    roots += __popcll(__ballot(r >= 0 && r == (int)k));
    int len = det_run_length(r, x, lane);
    // A component that fills much of the frame owns most runs of most waves, and every one of their atomics would go to its one
    // counter: the root of the wave's first run is added once for the whole wave -- its pixels in the wave are its runs' lengths
    // summed -- and only the runs of other roots add on their own.
    const unsigned long long lead = __ballot(len != 0);
    if (lead) {  // wave-uniform
      const int first = __ffsll((long long)lead) - 1;
      const int r0 = __shfl(r, first);
      const unsigned long long same = __ballot(r == r0);
      if (r == r0) len = lane == first ? __popcll(same) : 0;
    }
    if (len) {
      const int old = atomicAdd(area + o + r, len);
      if (old < min_area && old + len >= min_area) list[o + atomicAdd(counters + 2 * i + 1, 1)] = r;  // at most one entry per root: < HW
    }
  }
  if (lane == 0 && roots) atomicAdd(counters + 2 * i, roots);
}

// (area, root) as one key: the larger key is the better candidate (the larger area, then the smaller root); 0: none (area >= 1 else)
__device__ __forceinline__ unsigned long long det_key(int area, int root) {
  return ((unsigned long long)(unsigned)area << 32) | (unsigned)(DET_NONE - root);
}

__global__ __launch_bounds__(256) void det_rank_kernel(const long long* __restrict__ offsets, int k, int* __restrict__ area,
                                                       const int* __restrict__ list, const int* __restrict__ counters,
                                                       long long* __restrict__ dets, long long* __restrict__ counts) {
  __shared__ unsigned long long swave[4], swin[DET_K];
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const size_t o = (size_t)offsets[i];
  const int kept = counters[2 * i + 1];
  unsigned long long prev = ~0ull;
  int written = 0;
  for (int round = 0; round < k; ++round) {  // block-uniform: prev and written are the same in every thread
    unsigned long long best = 0;
    for (int j = t; j < kept; j += 256) {
      const int r = list[o + j];
      const unsigned long long key = det_key(area[o + r], r);  // the counters are not modified before the last round is over
      if (key < prev && key > best) best = key;
    }
    for (int s = 32; s > 0; s >>= 1) {
      const unsigned long long other = __shfl_xor(best, s);
      if (other > best) best = other;
    }
    if (lane == 0) swave[t >> 6] = best;
    __syncthreads();
    best = swave[0];
    for (int w = 1; w < 4; ++w)
      if (swave[w] > best) best = swave[w];
    __syncthreads();
    if (best == 0) break;  // nothing worse than the previous winner is left
    if (t == 0) swin[round] = best;
    prev = best;
    ++written;
  }
  __syncthreads();
  for (int rank = t; rank < k; rank += 256) {
    long long* __restrict__ d = dets + ((size_t)i * k + rank) * UDET_DET_FIELDS;
    if (rank < written) {
      const unsigned long long key = swin[rank];
      const int root = DET_NONE - (int)(unsigned)(key & 0xffffffffu);
      d[0] = root; d[1] = (long long)(key >> 32);
      d[2] = DET_NONE; d[3] = DET_NONE; d[4] = 0; d[5] = 0; d[6] = 0; d[7] = 0; d[8] = 0;
      area[o + root] = -1 - rank;
    } else {
      d[0] = -1;
      for (int f = 1; f < UDET_DET_FIELDS; ++f) d[f] = 0;
    }
  }
  if (t == 0) { counts[3 * i] = counters[2 * i]; counts[3 * i + 1] = kept; counts[3 * i + 2] = written; }
}

__global__ __launch_bounds__(256) void det_accum_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ score,
                                                        const long long* __restrict__ offsets, const int* __restrict__ hw, int k,
                                                        const int* __restrict__ area, long long* __restrict__ dets) {
  __shared__ int sbox[DET_K * 4];                  // y0, x0 (min), y1, x1 (max)
  __shared__ unsigned long long ssum[DET_K * 3];   // sum_y, sum_x, score_sum
  const int i = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int W = hw[2 * i + 1];
  const long long HW = (long long)hw[2 * i] * W;
  const size_t o = (size_t)offsets[i];
  for (int j = t; j < k * 4; j += 256) sbox[j] = (j & 2) ? 0 : DET_NONE;
  for (int j = t; j < k * 3; j += 256) ssum[j] = 0;
  __syncthreads();
  for (long long base = (long long)blockIdx.x * 256; base < HW; base += (long long)gridDim.x * 256) {  // block-uniform bounds
    const long long p = base + t;
    const bool valid = p < HW;
    const int v = valid ? labels[o + p] : 0;
    int rank = -1;
    if (v >= 1 && v <= HW) {
      const int a = area[o + v - 1];
      if (a < 0) rank = -1 - a;  // < k: written by det_rank_kernel
    }
    const int y = valid ? (int)p / W : 0, x = valid ? (int)p - y * W : 0;  // HW < 2^31
    // the score bytes of a run: an inclusive scan over the wave, the run's end minus what lies before its first lane
    const int sc = (rank >= 0 && score) ? score[o + p] : 0;
    int scan = sc;
    for (int s = 1; s < 64; s <<= 1) {
      const int up = __shfl_up(scan, s);
      if (lane >= s) scan += up;
    }
    const int len = det_run_length(rank, x, lane);
    const int at_end = __shfl(scan, len ? lane + len - 1 : lane);
    if (len) {
      atomicMin(sbox + 4 * rank, y);
      atomicMin(sbox + 4 * rank + 1, x);
      atomicMax(sbox + 4 * rank + 2, y + 1);
      atomicMax(sbox + 4 * rank + 3, x + len);
      atomicAdd(ssum + 3 * rank, (unsigned long long)len * y);
      atomicAdd(ssum + 3 * rank + 1, (unsigned long long)len * x + (unsigned long long)(len * (len - 1) / 2));
      if (score) atomicAdd(ssum + 3 * rank + 2, (unsigned long long)(at_end - scan + sc));
    }
  }
  __syncthreads();
  // one global atomic per touched value of a touched row; every value is >= 0, so the unsigned 64-bit forms order them as int64 does
  for (int j = t; j < k * DET_ACC; j += 256) {
    const int rank = j / DET_ACC, f = j - rank * DET_ACC;
    if (sbox[4 * rank] == DET_NONE) continue;  // no pixel of this winner in this workgroup
    unsigned long long* d = (unsigned long long*)(dets + ((size_t)i * k + rank) * UDET_DET_FIELDS + 2 + f);
    if (f < 2) atomicMin(d, (unsigned long long)sbox[4 * rank + f]);
    else if (f < 4) atomicMax(d, (unsigned long long)sbox[4 * rank + f]);
    else if (ssum[3 * rank + f - 4]) atomicAdd(d, ssum[3 * rank + f - 4]);
  }
}

// workspace: per-sample counters (roots, kept; int32), then the area counters and the kept-root lists (int32 per pixel of the packed buffer)
static inline size_t det_counter_bytes(int n) { return (size_t)n * 2 * sizeof(int); }
size_t component_boxes_workspace_bytes(size_t total_pixels, int n) { return det_counter_bytes(n) + 2 * total_pixels * sizeof(int); }

int launch_component_boxes_ragged(const int* labels, const unsigned char* score, int n, const long long* offsets, const int* hw, int max_h,
                                  int max_w, size_t total_pixels, int min_area, int k, long long* dets, long long* counts, void* workspace,
                                  hipStream_t s) {
  const long nb = ((long)max_h * max_w + 256 * DET_PPT - 1) / (256 * DET_PPT);
  const size_t nz = (total_pixels + 256 * DET_PPT - 1) / (256 * DET_PPT);
  if (nb > 0x7fffffffL) { set_error("component_boxes_ragged: frame too large"); return UDET_ERR_SHAPE; }
  int* counters = (int*)workspace;
  int* area = (int*)((char*)workspace + det_counter_bytes(n));
  int* list = area + total_pixels;
  hipLaunchKernelGGL(det_init_kernel, dim3((unsigned)(nz > 65536 ? 65536 : nz)), dim3(256), 0, s, area, total_pixels, counters, n);
  hipLaunchKernelGGL(det_area_kernel, dim3((unsigned)nb, n), dim3(256), 0, s, labels, offsets, hw, min_area, area, list, counters);
  hipLaunchKernelGGL(det_rank_kernel, dim3(n), dim3(256), 0, s, offsets, k, area, list, counters, dets, counts);
  hipLaunchKernelGGL(det_accum_kernel, dim3((unsigned)nb, n), dim3(256), 0, s, labels, score, offsets, hw, k, area, dets);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

// ---- udet_draw_boxes_ragged ---------------------------------------------------------------------------------------------------------
// One workgroup per (row of dets, sample): the four strips of the box's frame, each clipped to the box, painted with plain byte stores.
// Where strips or boxes overlap the bytes written are equal.  The box is clipped to its sample's frame and the row count to k, so
// whatever dets / counts hold nothing is written outside a sample.
__device__ __forceinline__ void det_paint(unsigned char* __restrict__ img, int W, int ya, int yb, int xa, int xb, unsigned rgb, int t) {
  const int w = xb - xa;
  if (w <= 0 || yb <= ya) return;
  const long long cells = (long long)(yb - ya) * w;
  for (long long c = t; c < cells; c += 256) {
    const int y = ya + (int)(c / w), x = xa + (int)(c % w);
    unsigned char* __restrict__ q = img + 3 * ((size_t)y * W + x);
    q[0] = (unsigned char)(rgb >> 16); q[1] = (unsigned char)(rgb >> 8); q[2] = (unsigned char)rgb;
  }
}

__global__ __launch_bounds__(256) void det_draw_kernel(unsigned char* __restrict__ rgb, const long long* __restrict__ offsets,
                                                       const int* __restrict__ hw, const long long* __restrict__ dets,
                                                       const long long* __restrict__ counts, int k, int th, unsigned colour) {
  const int i = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
  if ((long long)b >= counts[3 * i + 2]) return;  // block-uniform; b < k by the grid
  const long long* __restrict__ d = dets + ((size_t)i * k + b) * UDET_DET_FIELDS;
  if (d[0] < 0) return;
  const int H = hw[2 * i], W = hw[2 * i + 1];
  const long long ly0 = d[2], lx0 = d[3], ly1 = d[4], lx1 = d[5];
  const int y0 = (int)(ly0 < 0 ? 0 : ly0 > H ? H : ly0), y1 = (int)(ly1 < 0 ? 0 : ly1 > H ? H : ly1);
  const int x0 = (int)(lx0 < 0 ? 0 : lx0 > W ? W : lx0), x1 = (int)(lx1 < 0 ? 0 : lx1 > W ? W : lx1);
  if (y1 <= y0 || x1 <= x0) return;
  unsigned char* __restrict__ img = rgb + 3 * (size_t)offsets[i];
  const int ta = min(y0 + th, y1), bb = max(y1 - th, ta);  // rows [y0, ta) and [bb, y1) are full lines; between them the two side strips
  det_paint(img, W, y0, ta, x0, x1, colour, t);
  det_paint(img, W, bb, y1, x0, x1, colour, t);
  det_paint(img, W, ta, bb, x0, min(x0 + th, x1), colour, t);
  det_paint(img, W, ta, bb, max(x1 - th, x0), x1, colour, t);
}

int launch_draw_boxes_ragged(unsigned char* rgb, int n, const long long* offsets, const int* hw, const long long* dets,
                             const long long* counts, int k, int thickness, unsigned colour, hipStream_t s) {
  hipLaunchKernelGGL(det_draw_kernel, dim3(k, n), dim3(256), 0, s, rgb, offsets, hw, dets, counts, k, thickness, colour);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
