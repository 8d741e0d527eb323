// Detections linked into tracks across consecutive frames: udet_link_detections_ragged takes the labels components.hip
// wrote for n frames (packed layout, sample i = H_i x W_i int32 at offsets[i]) and the dets / counts detections.hip wrote for them, counts
// for every linked frame the pixels its rows share with the rows of the frame before it, matches the rows greedily by mask IoU and hands
// out track ids per sequence; udet_draw_track_boxes_ragged paints the boxes in the colour of their track.  Four launches for the link
// however many frames, sequences and components there are:
//   1. link_init_kernel     zeroes `inter`, writes every row's rank at its root into the workspace (one int32 per pixel, written at the
//                           winners' roots only and never zeroed: a lookup counts only when the row it names holds that root) and decides
//                           `linked`
//   2. link_overlap_kernel  every pixel of every linked frame: two labels, two lookups, the pair (a, b) of ranks; one LDS atomic per
//                           horizontal run of a wave into the workgroup's k x k histogram, then one 64-bit integer atomic per non-zero
//                           entry straight into `inter`
//   3. link_match_kernel    one workgroup per linked frame: the candidates (inter > 0, IoU at or above the threshold) into LDS, then at most
//                           min(rows_p, rows_c) rounds of a block arg-max over the entries whose rows are both free
//   4. link_ids_kernel      one wave per sequence (the wave of the sequence's first frame; the others leave at once), one lane per row:
//                           a matched row takes its predecessor's id by a shuffle, the unmatched rows the next free ids by a ballot prefix
// Integer work only, no workgroup waits for another: the outputs are exact, identical from run to run and for a sequence alone or inside
// a batch.  A label outside 1..H_i*W_i is background and a root outside 0..H_i*W_i-1 is not entered, so nothing indexes outside its own
// sample whatever labels and dets hold; every other index comes from offsets / hw, which the caller validates on the host
// (native_results.link_detections), and from ranks clamped to k.  udet_link_detections_gap_ragged (below the four
// kernels) adds the bridge across frames in which a component is missing: six launches, the same properties.
// udet_link_detections_motion_ragged / udet_link_detections_gap_motion_ragged are the same launches with the overlap pass
// of stage 1 in its MOTION form: the predecessor's label is read where a per-pixel displacement (csrc/motion.hip) says the pixel came from.
#include "common.h"
#include "elementwise.h"
#include "track_rows.h"  // link_rows, link_enter_roots: shared with instances.hip
#include "wave_runs.h"

namespace udet {

#define LINK_PPT 16    // pixels per thread of the overlap grid: 4096 pixels per workgroup and pass amortise the flush of k x k entries
#define LINK_K UDET_DET_MAX_K
#define LINK_NONE 0x7fffffff

static_assert(LINK_K <= 64, "one lane per row in link_ids_kernel");

// What a frame is linked against: the frame before it in the call, or the carried frame for the call's first one.
struct LinkCarry {
  const int* labels;        // carry_h x carry_w, or nullptr: no carried frame
  const long long* dets;    // [k][UDET_DET_FIELDS]
  const long long* counts;  // [3]
  const int* ids;           // [k]
  const int* next_id;       // [1]
  int h, w;
};

__global__ __launch_bounds__(256) void link_init_kernel(int n, const long long* __restrict__ offsets, const int* __restrict__ hw,
                                                        size_t total_pixels, const long long* __restrict__ dets,
                                                        const long long* __restrict__ counts, int k, const int* __restrict__ link,
                                                        LinkCarry carry, unsigned long long* __restrict__ inter,
                                                        int* __restrict__ linked, int* __restrict__ lookup) {
  const size_t stride = (size_t)gridDim.x * 256, g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t cells = (size_t)n * k * k;
  for (size_t j = g; j < cells; j += stride) inter[j] = 0;
  for (size_t j = g; j < (size_t)n * k; j += stride) {
    const int i = (int)(j / k), r = (int)(j - (size_t)i * k);
    link_enter_roots(dets + (size_t)i * k * UDET_DET_FIELDS, link_rows(counts + 3 * i, k), (long long)hw[2 * i] * hw[2 * i + 1],
                     lookup + offsets[i], r);
  }
  if (carry.labels)
    for (size_t r = g; r < (size_t)k; r += stride)
      link_enter_roots(carry.dets, link_rows(carry.counts, k), (long long)carry.h * carry.w, lookup + total_pixels, (int)r);
  for (size_t i = g; i < (size_t)n; i += stride) {
    const int H = hw[2 * i], W = hw[2 * i + 1];
    const bool same = i ? (hw[2 * i - 2] == H && hw[2 * i - 1] == W) : (carry.labels && carry.h == H && carry.w == W);
    linked[i] = (link[i] != 0 && same) ? 1 : 0;
  }
}

// The rows of one frame of a sequence against the rows of an earlier one of its size: the workgroup's share of the pixels into its k x k
// histogram, then one 64-bit atomic per non-zero entry into out [k][k].  at_p / at_c: where the two frames' ranks lie in the lookup.
struct LinkSide {
  const int* labels;
  const long long* dets;
  int rows;
  size_t at;
};

// MOTION: the predecessor's label is read where disp says the pixel came from -- dx in the low 16 bits, dy in the high
// 16, both signed; the source is tested in 2-D against the H x W frame before it becomes an address, and a source outside the frame is
// background.  Without MOTION disp and H are not looked at and the pass is what it was.
template <bool MOTION>
__device__ __forceinline__ void link_overlap_pass(LinkSide fp, LinkSide fc, int H, int W, long long HW, int k,
                                                  const int* __restrict__ lookup, const int* __restrict__ disp,
                                                  unsigned long long* __restrict__ out, int* __restrict__ lds) {
  const int t = threadIdx.x, lane = t & 63;
  int* __restrict__ hist = lds;  // hist [k * k], root_p [k], root_c [k]
  int* __restrict__ root_p = lds + k * k;
  int* __restrict__ root_c = root_p + k;
  const int* __restrict__ lab_p = fp.labels;
  const int* __restrict__ lab_c = fc.labels;
  const int rows_p = fp.rows, rows_c = fc.rows;
  const size_t op = fp.at, oc = fc.at;
  for (int j = t; j < k * k; j += 256) hist[j] = 0;
  for (int j = t; j < k; j += 256) {
    root_p[j] = j < rows_p ? (int)fp.dets[(size_t)j * UDET_DET_FIELDS] : -1;  // a root >= 2^31 matches no label
    root_c[j] = j < rows_c ? (int)fc.dets[(size_t)j * UDET_DET_FIELDS] : -1;
  }
  __syncthreads();
  for (long long base = (long long)blockIdx.x * 256; base < HW; base += (long long)gridDim.x * 256) {  // block-uniform bounds
    const long long p = base + t;
    const bool valid = p < HW;
    int vp = 0;
    const int vc = valid ? lab_c[p] : 0;
    if (MOTION) {
      if (valid) {
        const int dv = disp[p];
        const long long y = p / W;
        const long long xs = (p - y * W) + (short)(dv & 0xffff), ys = y + (dv >> 16);  // |dx|, |dy| <= 2^15: no overflow
        if (xs >= 0 && xs < W && ys >= 0 && ys < H) vp = lab_p[ys * W + xs];           // 0 <= ys W + xs < HW
      }
    } else {
      vp = valid ? lab_p[p] : 0;
    }
    int a = -1, b = -1;
    if (vp >= 1 && vp <= HW && vc >= 1 && vc <= HW) {
      const int ra = lookup[op + vp - 1], rb = lookup[oc + vc - 1];  // never zeroed: only a rank whose row holds this root counts
      if ((unsigned)ra < (unsigned)rows_p && root_p[ra] == vp - 1) a = ra;
      if ((unsigned)rb < (unsigned)rows_c && root_c[rb] == vc - 1) b = rb;
    }
    const int pair = (a >= 0 && b >= 0) ? a * k + b : -1;
    const int len = det_run_length(pair, valid ? (int)(p % W) : 0, lane);
    if (len) atomicAdd(hist + pair, len);  // a workgroup sees fewer than 2^31 pixels
  }
  __syncthreads();
  for (int j = t; j < k * k; j += 256)
    if (hist[j]) atomicAdd(out + j, (unsigned long long)hist[j]);
}

// disp: one packed displacement per pixel of the batch, laid out like labels (MOTION only; a frame that is not linked reads none of it).
template <bool MOTION>
__global__ __launch_bounds__(256) void link_overlap_kernel(const int* __restrict__ labels, const long long* __restrict__ offsets,
                                                           const int* __restrict__ hw, size_t total_pixels,
                                                           const long long* __restrict__ dets, const long long* __restrict__ counts, int k,
                                                           LinkCarry carry, const int* __restrict__ linked, const int* __restrict__ lookup,
                                                           const int* __restrict__ disp, unsigned long long* __restrict__ inter) {
  extern __shared__ int link_lds[];
  const int i = blockIdx.y;
  if (!linked[i]) return;  // block-uniform; a linked frame 0 has a carried frame of its size
  const int W = hw[2 * i + 1];
  const long long HW = (long long)hw[2 * i] * W;  // the predecessor's too
  const long long* __restrict__ dets_c = dets + (size_t)i * k * UDET_DET_FIELDS;
  const LinkSide fc = {labels + offsets[i], dets_c, link_rows(counts + 3 * i, k), (size_t)offsets[i]};
  const LinkSide fp = i ? LinkSide{labels + offsets[i - 1], dets_c - (size_t)k * UDET_DET_FIELDS, link_rows(counts + 3 * i - 3, k),
                                   (size_t)offsets[i - 1]}
                        : LinkSide{carry.labels, carry.dets, link_rows(carry.counts, k), total_pixels};
  link_overlap_pass<MOTION>(fp, fc, hw[2 * i], W, HW, k, lookup, MOTION ? disp + offsets[i] : nullptr, inter + (size_t)i * k * k, link_lds);
}

// (inter, union, entry) of the better of two candidates: the larger inter / union by 64-bit cross-multiplication (inter < 2^31, union <
// 2^32), ties to the smaller entry a * k + b -- the smaller a, then the smaller b.  (0, 1, LINK_NONE): none.
__device__ __forceinline__ bool link_better(int i1, unsigned u1, int j1, int i2, unsigned u2, int j2) {
  const unsigned long long p1 = (unsigned long long)i1 * u2, p2 = (unsigned long long)i2 * u1;
  return p1 > p2 || (p1 == p2 && j1 < j2);
}

// The best of the 256 threads' candidates, in every thread: shuffles inside a wave, then the four waves' winners through LDS (wi, wu,
// wj: [4]).  Holds one __syncthreads; the caller's next barrier separates this round's reads of wi / wu / wj from the next round's writes.
__device__ __forceinline__ void link_block_best(int& bi, unsigned& bu, int& bj, int* wi, unsigned* wu, int* wj) {
  const int t = threadIdx.x;
  for (int s = 32; s > 0; s >>= 1) {
    const int oi = __shfl_xor(bi, s), oj = __shfl_xor(bj, s);
    const unsigned ou = __shfl_xor(bu, s);
    if (link_better(oi, ou, oj, bi, bu, bj)) { bi = oi; bu = ou; bj = oj; }
  }
  if ((t & 63) == 0) { wi[t >> 6] = bi; wu[t >> 6] = bu; wj[t >> 6] = bj; }
  __syncthreads();
  bi = wi[0]; bu = wu[0]; bj = wj[0];
  for (int w = 1; w < 4; ++w)
    if (link_better(wi[w], wu[w], wj[w], bi, bu, bj)) { bi = wi[w]; bu = wu[w]; bj = wj[w]; }
}

__global__ __launch_bounds__(256) void link_match_kernel(const long long* __restrict__ dets, const long long* __restrict__ counts, int k,
                                                         LinkCarry carry, const int* __restrict__ linked,
                                                         const long long* __restrict__ inter, int permille, int* __restrict__ match) {
  extern __shared__ int link_lds[];  // inter of the candidates [k * k] (0: none), their unions [k * k], free_p [k], free_c [k], match [k]
  __shared__ int wi[4], wj[4];
  __shared__ unsigned wu[4];
  const int i = blockIdx.x, t = threadIdx.x;
  int* __restrict__ sint = link_lds;
  unsigned* __restrict__ suni = (unsigned*)(link_lds + k * k);
  int* __restrict__ free_p = link_lds + 2 * k * k;
  int* __restrict__ free_c = free_p + k;
  int* __restrict__ smatch = free_c + k;
  if (!linked[i]) {  // block-uniform
    for (int b = t; b < k; b += 256) match[(size_t)i * k + b] = -1;
    return;
  }
  const long long* __restrict__ dets_c = dets + (size_t)i * k * UDET_DET_FIELDS;
  const long long* __restrict__ dets_p = i ? dets_c - (size_t)k * UDET_DET_FIELDS : carry.dets;
  const int rows_c = link_rows(counts + 3 * i, k), rows_p = link_rows(i ? counts + 3 * i - 3 : carry.counts, k);
  for (int j = t; j < k * k; j += 256) {
    const int a = j / k, b = j - a * k;
    const long long v = inter[(size_t)i * k * k + j];
    int keep = 0;
    unsigned uni = 1;
    if (a < rows_p && b < rows_c && v > 0 && v <= 0x7fffffffLL) {
      const long long u = dets_p[(size_t)a * UDET_DET_FIELDS + 1] + dets_c[(size_t)b * UDET_DET_FIELDS + 1] - v;  // area_a + area_b - inter
      if (u > 0 && u <= 0xffffffffLL && 1000 * v >= (long long)permille * u) { keep = (int)v; uni = (unsigned)u; }
    }
    sint[j] = keep;
    suni[j] = uni;
  }
  for (int j = t; j < k; j += 256) { free_p[j] = 1; free_c[j] = 1; smatch[j] = -1; }
  __syncthreads();
  const int rounds = rows_p < rows_c ? rows_p : rows_c;
  for (int round = 0; round < rounds; ++round) {  // block-uniform: every thread sees the same winner
    int bi = 0, bj = LINK_NONE;
    unsigned bu = 1;
    for (int j = t; j < k * k; j += 256) {
      const int v = sint[j];
      if (!v) continue;
      const int a = j / k;
      if (free_p[a] && free_c[j - a * k] && link_better(v, suni[j], j, bi, bu, bj)) { bi = v; bu = suni[j]; bj = j; }
    }
    link_block_best(bi, bu, bj, wi, wu, wj);
    if (bi == 0) break;  // no candidate between free rows is left
    if (t == 0) {
      const int a = bj / k, b = bj - a * k;
      smatch[b] = a; free_p[a] = 0; free_c[b] = 0;
    }
    __syncthreads();
  }
  __syncthreads();
  for (int b = t; b < k; b += 256) match[(size_t)i * k + b] = smatch[b];
}

__global__ __launch_bounds__(64) void link_ids_kernel(int n, const long long* __restrict__ counts, int k, LinkCarry carry,
                                                      const int* __restrict__ linked, const int* __restrict__ match,
                                                      int* __restrict__ ids, int* __restrict__ seq_tracks, int* __restrict__ next_id_out) {
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s > 0 && linked[s]) return;  // wave-uniform: only the wave of a sequence's first frame walks it
  int c = s, next, prev;
  if (linked[s]) {  // frame 0 continues the carried frame
    prev = lane < k ? carry.ids[lane] : -1;
    next = carry.next_id[0];
  } else {
    const int rows = link_rows(counts + 3 * s, k);
    prev = lane < rows ? lane : -1;
    next = rows;
    if (lane < k) ids[(size_t)s * k + lane] = prev;
    if (lane == 0) seq_tracks[s] = 0;
    ++c;
  }
  for (; c < n && linked[c]; ++c) {  // wave-uniform
    const int rows = link_rows(counts + 3 * c, k);
    int m = lane < k ? match[(size_t)c * k + lane] : -1;
    if (m < 0 || m >= k) m = -1;
    const int inherited = __shfl(prev, m < 0 ? 0 : m);
    const bool fresh = lane < rows && m < 0;
    const unsigned long long mask = __ballot(fresh);
    int id = -1;
    if (lane < rows) id = m >= 0 ? inherited : next + __popcll(mask & ((1ull << lane) - 1ull));
    next += __popcll(mask);
    if (lane < k) ids[(size_t)c * k + lane] = id;
    if (lane == 0) seq_tracks[c] = 0;
    prev = id;
  }
  if (lane == 0) {  // c - 1 >= s: the sequence's last frame within the call (the same lane wrote its 0 above)
    seq_tracks[c - 1] = next;
    if (c == n) next_id_out[0] = next;
  }
}

size_t link_detections_workspace_bytes(size_t total_pixels, int carry_h, int carry_w) {
  return (total_pixels + (size_t)carry_h * carry_w) * sizeof(int);
}

int launch_link_detections_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                  size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                  const int* carry_labels, int carry_h, int carry_w, const long long* carry_dets,
                                  const long long* carry_counts, const int* carry_ids, const int* carry_next_id, int min_iou_permille,
                                  long long* inter, int* match, int* ids, int* linked, int* seq_tracks, int* next_id, const int* disp,
                                  void* workspace, hipStream_t s) {
  const long nb = ((long)max_h * max_w + 256 * LINK_PPT - 1) / (256 * LINK_PPT);
  if (nb > 0x7fffffffL) { set_error("link_detections_ragged: frame too large"); return UDET_ERR_SHAPE; }
  const LinkCarry carry = {carry_labels, carry_dets, carry_counts, carry_ids, carry_next_id, carry_h, carry_w};
  int* lookup = (int*)workspace;
  const auto overlap = disp ? link_overlap_kernel<true> : link_overlap_kernel<false>;  // disp = nullptr: the co-located link
  const size_t nz = ((size_t)n * k * k + 255) / 256;
  const size_t lds_overlap = ((size_t)k * k + 2 * k) * sizeof(int), lds_match = (2 * (size_t)k * k + 3 * k) * sizeof(int);
  hipLaunchKernelGGL(link_init_kernel, dim3((unsigned)(nz > 65536 ? 65536 : nz)), dim3(256), 0, s, n, offsets, hw, total_pixels, dets,
                     counts, k, link, carry, (unsigned long long*)inter, linked, lookup);
  hipLaunchKernelGGL(overlap, dim3((unsigned)nb, n), dim3(256), lds_overlap, s, labels, offsets, hw, total_pixels, dets, counts, k, carry,
                     linked, lookup, disp, (unsigned long long*)inter);
  hipLaunchKernelGGL(link_match_kernel, dim3(n), dim3(256), lds_match, s, dets, counts, k, carry, linked, inter, min_iou_permille, match);
  hipLaunchKernelGGL(link_ids_kernel, dim3(n), dim3(64), 0, s, n, counts, k, carry, linked, match, ids, seq_tracks, next_id);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

// ---- udet_link_detections_gap_ragged --------------------------------------------------------------------------------
// A row without a predecessor in the frame before it may continue a track that ended up to max_gap frames earlier.  Stage 1 is the three
// launches above, unchanged (the carried frame is the history's last one); then
//   gap_init_kernel     zeroes gap_inter and enters the rows of the older history frames in the lookup
//   gap_overlap_kernel  link_overlap_pass for (frame c, distance d) with d on the grid's z axis: frame c against frame c - d
//   gap_walk_kernel     one workgroup per sequence (that of its first frame in the call; the others leave at once) walks the frames in
//                       order with the open flags, ids and areas of the last max_gap + 1 frames in a ring in LDS: stage-1 rows inherit,
//                       then at most `orphans` rounds of a block arg-max over the thresholded gap candidates between free orphans and
//                       open rows, then the fresh ids by a ballot prefix
// Six launches whatever n, the sequences, the components and max_gap.  Frame c - d with c - d < 0 is history frame m + c - d; the
// history's ranks lie behind the batch's in the lookup, newest first (frame j at total_pixels + (m - 1 - j) h w), so that the carried
// frame is where the stage-1 kernels look for it.
#define GAP_RING (UDET_TRACK_MAX_GAP + 2)  // frames c - max_gap - 1 .. c

struct LinkHistory {
  const int* labels;        // [m][h * w], or nullptr: no history
  const long long* dets;    // [m][k][UDET_DET_FIELDS]
  const long long* counts;  // [m][3]
  const int* ids;           // [m][k]
  int* open;                // [m][k], in / out
  const int* next_id;       // [1]
  int m, h, w;
};

// Whether frame c - d belongs to frame c's sequence: the frames c - d + 1 .. c of the call are linked, and below frame 0 (reached only
// through a linked frame 0, so the history has its size) the history's m frames follow.
__device__ __forceinline__ bool gap_reaches(const int* __restrict__ linked, int c, int d, int m) {
  for (int j = 0; j < d && c - j >= 0; ++j)
    if (!linked[c - j]) return false;
  return c - d >= -m;
}

__device__ __forceinline__ int gap_slot(int f) { return (f + GAP_RING) % GAP_RING; }  // f >= -GAP_RING

__global__ __launch_bounds__(256) void gap_init_kernel(int n, int k, int max_gap, size_t total_pixels, LinkHistory hist,
                                                       unsigned long long* __restrict__ gap_inter, int* __restrict__ lookup) {
  const size_t stride = (size_t)gridDim.x * 256, g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t cells = (size_t)n * max_gap * k * k, frame = (size_t)hist.h * hist.w;
  for (size_t j = g; j < cells; j += stride) gap_inter[j] = 0;
  for (size_t j = g; j + k < (size_t)hist.m * k; j += stride) {  // the frames 0 .. m - 2: link_init_kernel entered the carried one
    const int f = (int)(j / k), r = (int)(j - (size_t)f * k);
    link_enter_roots(hist.dets + (size_t)f * k * UDET_DET_FIELDS, link_rows(hist.counts + 3 * f, k), (long long)frame,
                     lookup + total_pixels + (size_t)(hist.m - 1 - f) * frame, r);
  }
}

__global__ __launch_bounds__(256) void gap_overlap_kernel(const int* __restrict__ labels, const long long* __restrict__ offsets,
                                                          const int* __restrict__ hw, size_t total_pixels,
                                                          const long long* __restrict__ dets, const long long* __restrict__ counts, int k,
                                                          int max_gap, LinkHistory hist, const int* __restrict__ linked,
                                                          const int* __restrict__ lookup, unsigned long long* __restrict__ gap_inter) {
  extern __shared__ int link_lds[];
  const int c = blockIdx.y, d = blockIdx.z + 2, f = c - d;
  if (!gap_reaches(linked, c, d, hist.m)) return;  // block-uniform
  const int W = hw[2 * c + 1];
  const long long HW = (long long)hw[2 * c] * W;  // frame f's too
  const LinkSide fc = {labels + offsets[c], dets + (size_t)c * k * UDET_DET_FIELDS, link_rows(counts + 3 * c, k), (size_t)offsets[c]};
  const int j = hist.m + f;  // f < 0: the history's frame j, 0 <= j < m
  const LinkSide fp = f >= 0 ? LinkSide{labels + offsets[f], dets + (size_t)f * k * UDET_DET_FIELDS, link_rows(counts + 3 * f, k),
                                        (size_t)offsets[f]}
                             : LinkSide{hist.labels + (size_t)j * HW, hist.dets + (size_t)j * k * UDET_DET_FIELDS,
                                        link_rows(hist.counts + 3 * j, k), total_pixels + (size_t)(hist.m - 1 - j) * HW};
  link_overlap_pass<false>(fp, fc, 0, W, HW, k, lookup, nullptr, gap_inter + ((size_t)c * max_gap + (d - 2)) * k * k, link_lds);
}

// A row of frame f (f < 0: of the history) has found its successor.
__device__ __forceinline__ void gap_close(int f, int a, int k, LinkHistory hist, int* __restrict__ open) {
  if (f >= 0) open[(size_t)f * k + a] = 0;
  else hist.open[(size_t)(hist.m + f) * k + a] = 0;
}

__global__ __launch_bounds__(256) void gap_walk_kernel(int n, const long long* __restrict__ dets, const long long* __restrict__ counts, int k,
                                                       int max_gap, LinkHistory hist, const int* __restrict__ linked,
                                                       const int* __restrict__ match, const long long* __restrict__ gap_inter, int permille,
                                                       int* __restrict__ ids, int* __restrict__ back, int* __restrict__ prev,
                                                       int* __restrict__ open, int* __restrict__ seq_tracks, int* __restrict__ next_id_out) {
  __shared__ int sopen[GAP_RING][LINK_K], sid[GAP_RING][LINK_K];  // per frame of the ring and row: still open, its track id
  __shared__ long long sarea[GAP_RING][LINK_K];
  __shared__ int sorph[LINK_K], sback[LINK_K], sprev[LINK_K];     // per row of the frame: a free orphan, the bridge it took (0: none)
  __shared__ int wi[4], wj[4];
  __shared__ unsigned wu[4];
  const int s = blockIdx.x, t = threadIdx.x, b = t & 63;
  if (s > 0 && linked[s]) return;  // block-uniform: only the workgroup of a sequence's first frame walks it
  // Every wave does the per-row work on lane = row and so holds the same `next`; wave 0 (t = b) writes.
  int c = s, next, avail;  // avail: the frames of the sequence before frame c, the history's included
  if (linked[s]) {         // frame 0 continues the history
    for (int j = 0; j < hist.m; ++j) {
      const int rows = link_rows(hist.counts + 3 * j, k), sl = gap_slot(j - hist.m);
      if (t < k) {
        sopen[sl][t] = t < rows && hist.open[(size_t)j * k + t] != 0;
        sid[sl][t] = hist.ids[(size_t)j * k + t];
        sarea[sl][t] = t < rows ? hist.dets[((size_t)j * k + t) * UDET_DET_FIELDS + 1] : 0;
      }
    }
    next = hist.next_id[0];
    avail = hist.m;
  } else {
    const int rows = link_rows(counts + 3 * s, k), sl = gap_slot(s);
    if (t < k) {
      const int id = t < rows ? t : -1;
      sopen[sl][t] = t < rows;
      sid[sl][t] = id;
      sarea[sl][t] = t < rows ? dets[((size_t)s * k + t) * UDET_DET_FIELDS + 1] : 0;
      ids[(size_t)s * k + t] = id; back[(size_t)s * k + t] = 0; prev[(size_t)s * k + t] = -1; open[(size_t)s * k + t] = t < rows;
    }
    if (t == 0) seq_tracks[s] = 0;
    next = rows;
    avail = 1;
    ++c;
  }
  __syncthreads();
  for (; c < n && linked[c]; ++c, ++avail) {  // block-uniform
    const int rows = link_rows(counts + 3 * c, k), sc = gap_slot(c), sp = gap_slot(c - 1);
    int m = b < rows ? match[(size_t)c * k + b] : -1;
    if (m < 0 || m >= k) m = -1;
    const bool orphan = b < rows && m < 0;
    const int orphans = __popcll(__ballot(orphan));
    int id = m >= 0 ? sid[sp][m] : -1, bk = m >= 0 ? 1 : 0;
    if (t < k) {
      sopen[sc][t] = t < rows;
      sarea[sc][t] = t < rows ? dets[((size_t)c * k + t) * UDET_DET_FIELDS + 1] : 0;
      sorph[t] = orphan; sback[t] = 0; sprev[t] = -1;
      open[(size_t)c * k + t] = t < rows;
      if (m >= 0) { sopen[sp][m] = 0; gap_close(c - 1, m, k, hist, open); }  // stage 1 comes first: a bridge never undoes it
    }
    __syncthreads();
    const int dmax = avail < max_gap + 1 ? avail : max_gap + 1;
    for (int round = 0; round < orphans && dmax >= 2; ++round) {  // block-uniform: every thread sees the same winner
      int bi = 0, bj = LINK_NONE;
      unsigned bu = 1;
      for (int d = 2; d <= dmax; ++d) {
        const int sa = gap_slot(c - d);
        const long long* __restrict__ g = gap_inter + ((size_t)c * max_gap + (d - 2)) * k * k;
        for (int j = t; j < k * k; j += 256) {
          const int a = j / k, bb = j - a * k;
          if (!sorph[bb] || !sopen[sa][a]) continue;
          const long long v = g[j];
          if (v <= 0 || v > 0x7fffffffLL) continue;
          const long long u = sarea[sa][a] + sarea[sc][bb] - v;  // area_a + area_b - gap_inter
          const int key = (d - 2) * k * k + j;                   // ties: the smaller d, then the smaller a, then the smaller b
          if (u > 0 && u <= 0xffffffffLL && 1000 * v >= (long long)permille * u && link_better((int)v, (unsigned)u, key, bi, bu, bj)) {
            bi = (int)v; bu = (unsigned)u; bj = key;
          }
        }
      }
      link_block_best(bi, bu, bj, wi, wu, wj);
      if (bi == 0) break;  // no candidate between a free orphan and an open row is left
      if (t == 0) {
        const int d = bj / (k * k) + 2, j = bj - (d - 2) * k * k, a = j / k, bb = j - a * k;
        sorph[bb] = 0; sback[bb] = d; sprev[bb] = a;
        sopen[gap_slot(c - d)][a] = 0;
        gap_close(c - d, a, k, hist, open);
      }
      __syncthreads();
    }
    if (orphan && sback[b]) { bk = sback[b]; m = sprev[b]; id = sid[gap_slot(c - bk)][m]; }
    const bool fresh = orphan && bk == 0;
    const unsigned long long mask = __ballot(fresh);
    if (fresh) id = next + __popcll(mask & ((1ull << b) - 1ull));
    next += __popcll(mask);
    if (t < k) {
      ids[(size_t)c * k + t] = id; back[(size_t)c * k + t] = bk; prev[(size_t)c * k + t] = m;
      sid[sc][t] = id;
    }
    if (t == 0) seq_tracks[c] = 0;
    __syncthreads();
  }
  if (t == 0) {  // c - 1 >= s: the sequence's last frame within the call (the same thread wrote its 0 above)
    seq_tracks[c - 1] = next;
    if (c == n) next_id_out[0] = next;
  }
}

size_t link_detections_gap_workspace_bytes(size_t total_pixels, int m, int hist_h, int hist_w) {
  return (total_pixels + (size_t)m * hist_h * hist_w) * sizeof(int);
}

int launch_link_detections_gap_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                      size_t total_pixels, const long long* dets, const long long* counts, int k, const int* link,
                                      int max_gap, int m, const int* hist_labels, int hist_h, int hist_w, const long long* hist_dets,
                                      const long long* hist_counts, const int* hist_ids, int* hist_open, const int* hist_next_id,
                                      int min_iou_permille, long long* inter, int* match, int* ids, int* linked, int* seq_tracks,
                                      int* next_id, long long* gap_inter, int* back, int* prev, int* open, const int* disp,
                                      void* workspace, hipStream_t s) {
  const long nb = ((long)max_h * max_w + 256 * LINK_PPT - 1) / (256 * LINK_PPT);
  if (nb > 0x7fffffffL) { set_error("link_detections_gap_ragged: frame too large"); return UDET_ERR_SHAPE; }
  const LinkHistory hist = {hist_labels, hist_dets, hist_counts, hist_ids, hist_open, hist_next_id, m, hist_h, hist_w};
  const size_t last = m ? (size_t)(m - 1) : 0, frame = (size_t)hist_h * hist_w;  // stage 1 is linked against the history's last frame
  const LinkCarry carry = {m ? hist_labels + last * frame : nullptr, m ? hist_dets + last * k * UDET_DET_FIELDS : nullptr,
                           m ? hist_counts + 3 * last : nullptr, m ? hist_ids + last * k : nullptr, hist_next_id, hist_h, hist_w};
  int* lookup = (int*)workspace;
  const auto overlap = disp ? link_overlap_kernel<true> : link_overlap_kernel<false>;  // disp = nullptr: the co-located link
  const size_t nz = ((size_t)n * k * k + 255) / 256, ngz = nz * max_gap;
  const size_t lds_overlap = ((size_t)k * k + 2 * k) * sizeof(int), lds_match = (2 * (size_t)k * k + 3 * k) * sizeof(int);
  hipLaunchKernelGGL(link_init_kernel, dim3((unsigned)(nz > 65536 ? 65536 : nz)), dim3(256), 0, s, n, offsets, hw, total_pixels, dets,
                     counts, k, link, carry, (unsigned long long*)inter, linked, lookup);
  hipLaunchKernelGGL(gap_init_kernel, dim3((unsigned)(ngz > 65536 ? 65536 : ngz)), dim3(256), 0, s, n, k, max_gap, total_pixels, hist,
                     (unsigned long long*)gap_inter, lookup);
  hipLaunchKernelGGL(overlap, dim3((unsigned)nb, n), dim3(256), lds_overlap, s, labels, offsets, hw, total_pixels, dets, counts, k, carry,
                     linked, lookup, disp, (unsigned long long*)inter);
  hipLaunchKernelGGL(gap_overlap_kernel, dim3((unsigned)nb, n, max_gap), dim3(256), lds_overlap, s, labels, offsets, hw, total_pixels, dets,
                     counts, k, max_gap, hist, linked, lookup, (unsigned long long*)gap_inter);
  hipLaunchKernelGGL(link_match_kernel, dim3(n), dim3(256), lds_match, s, dets, counts, k, carry, linked, inter, min_iou_permille, match);
  hipLaunchKernelGGL(gap_walk_kernel, dim3(n), dim3(256), 0, s, n, dets, counts, k, max_gap, hist, linked, match, gap_inter,
                     min_iou_permille, ids, back, prev, open, seq_tracks, next_id);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

// ---- udet_draw_track_boxes_ragged ---------------------------------------------------------------------------------------------------
// One workgroup per (row of dets, sample), as det_draw_kernel: the four strips of the box's frame in the colour of the row's track.  A
// pixel that lies on the line of a painted lower-ranked box is skipped, so every pixel is written by the smallest rank that covers it,
// whatever order the workgroups run in.  Boxes are clipped to their sample's frame and the row count to k.
struct TrackBox { int y0, x0, y1, x1; };

__device__ __forceinline__ bool track_clip(const long long* __restrict__ d, int H, int W, TrackBox* b) {
  if (d[0] < 0) return false;
  const long long ly0 = d[2], lx0 = d[3], ly1 = d[4], lx1 = d[5];
  b->y0 = (int)(ly0 < 0 ? 0 : ly0 > H ? H : ly0); b->y1 = (int)(ly1 < 0 ? 0 : ly1 > H ? H : ly1);
  b->x0 = (int)(lx0 < 0 ? 0 : lx0 > W ? W : lx0); b->x1 = (int)(lx1 < 0 ? 0 : lx1 > W ? W : lx1);
  return b->y1 > b->y0 && b->x1 > b->x0;
}

__device__ __forceinline__ void track_paint(unsigned char* __restrict__ img, int W, int ya, int yb, int xa, int xb, unsigned rgb, int t,
                                            const int* __restrict__ lower, int n_lower, int th) {
  const int w = xb - xa;
  if (w <= 0 || yb <= ya) return;
  const long long cells = (long long)(yb - ya) * w;
  for (long long c = t; c < cells; c += 256) {
    const int y = ya + (int)(c / w), x = xa + (int)(c % w);
    bool hidden = false;
    for (int q = 0; q < n_lower && !hidden; ++q) {
      const int y0 = lower[4 * q], x0 = lower[4 * q + 1], y1 = lower[4 * q + 2], x1 = lower[4 * q + 3];  // an unpainted row: empty
      hidden = y >= y0 && y < y1 && x >= x0 && x < x1 && (y < y0 + th || y >= y1 - th || x < x0 + th || x >= x1 - th);
    }
    if (hidden) continue;
    unsigned char* __restrict__ q = img + 3 * ((size_t)y * W + x);
    q[0] = (unsigned char)(rgb >> 16); q[1] = (unsigned char)(rgb >> 8); q[2] = (unsigned char)rgb;
  }
}

__global__ __launch_bounds__(256) void track_draw_kernel(unsigned char* __restrict__ rgb, const long long* __restrict__ offsets,
                                                         const int* __restrict__ hw, const long long* __restrict__ dets,
                                                         const long long* __restrict__ counts, int k, const int* __restrict__ ids, int th,
                                                         const unsigned* __restrict__ palette, int palette_size) {
  __shared__ int lower[LINK_K * 4];
  const int i = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
  if (b >= link_rows(counts + 3 * i, k)) return;  // block-uniform; b < k by the grid
  const int id = ids[(size_t)i * k + b];
  if (id < 0) return;
  const int H = hw[2 * i], W = hw[2 * i + 1];
  TrackBox own;
  if (!track_clip(dets + ((size_t)i * k + b) * UDET_DET_FIELDS, H, W, &own)) return;
  for (int q = t; q < b; q += 256) {
    TrackBox lo;
    const bool painted = ids[(size_t)i * k + q] >= 0 && track_clip(dets + ((size_t)i * k + q) * UDET_DET_FIELDS, H, W, &lo);
    lower[4 * q] = painted ? lo.y0 : 0; lower[4 * q + 1] = painted ? lo.x0 : 0;
    lower[4 * q + 2] = painted ? lo.y1 : 0; lower[4 * q + 3] = painted ? lo.x1 : 0;
  }
  __syncthreads();
  const unsigned colour = palette[id % palette_size] & 0xffffffu;
  unsigned char* __restrict__ img = rgb + 3 * (size_t)offsets[i];
  const int ta = min(own.y0 + th, own.y1), bb = max(own.y1 - th, ta);  // rows [y0, ta) and [bb, y1) are full lines; between them the side strips
  track_paint(img, W, own.y0, ta, own.x0, own.x1, colour, t, lower, b, th);
  track_paint(img, W, bb, own.y1, own.x0, own.x1, colour, t, lower, b, th);
  track_paint(img, W, ta, bb, own.x0, min(own.x0 + th, own.x1), colour, t, lower, b, th);
  track_paint(img, W, ta, bb, max(own.x1 - th, own.x0), own.x1, colour, t, lower, b, th);
}

int launch_draw_track_boxes_ragged(unsigned char* rgb, int n, const long long* offsets, const int* hw, const long long* dets,
                                   const long long* counts, int k, const int* ids, int thickness, const unsigned* palette,
                                   int palette_size, hipStream_t s) {
  hipLaunchKernelGGL(track_draw_kernel, dim3(k, n), dim3(256), 0, s, rgb, offsets, hw, dets, counts, k, ids, thickness, palette,
                     palette_size);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
