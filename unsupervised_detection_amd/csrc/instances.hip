// Per-track instance maps and their picture, from what the link left on the device: udet_track_instance_maps_ragged
// writes for n frames (packed layout, sample i = H_i x W_i at offsets[i]) the byte map in which every pixel names its track, the pixels
// every row shares with the annotation and three counts per frame; udet_overlay_instances_ragged blends the map on the frames, every
// instance in its track's colour, with a contour wherever two different values meet.
//   1. inst_init_kernel           zeroes row_gt and frame_stats and writes every row's rank at its root into the workspace -- the lookup of
//                                 the link (track_rows.h): one int32 per pixel, never zeroed, a lookup counts only when the row it names
//                                 holds that root
//   2. inst_paint_kernel          one lane per pixel, a wave on 64 consecutive pixels of one sample: label, lookup, the row's value from LDS;
//                                 four lanes' bytes make one aligned 32-bit word of the map; the pixels of row r under the annotation go by
//                                 one LDS atomic per horizontal run of the wave (wave_runs.h) into the workgroup's k partials, the three
//                                 counts by ballots; then one 64-bit integer atomic per non-zero partial
//   3. overlay_instances_kernel   a 32 x 64 tile of one sample: the map's bytes with an edge-wide halo in LDS (coordinates clamped into the
//                                 frame, so that a position outside it never differs), the windowed minimum and maximum over the rows, then
//                                 over the columns, and the colour bytes through rgb_groups.h
// Two launches for the maps and one for the picture whatever n, k, the components and the sequences are; integer atomics only, no
// workgroup waits for another: identical from run to run and for a sample alone or inside a batch.  A label outside 1..H_i*W_i is
// background and a looked-up rank counts only below the frame's rows, so nothing indexes outside its own sample whatever labels, dets,
// counts, ids and the workspace hold; offsets / hw are validated by the host caller (native_instances.instance_maps).
#include <math.h>

#include "common.h"
#include "host_checks.h"
#include "packed_bytes.h"
#include "rgb_groups.h"
#include "track_rows.h"
#include "wave_runs.h"

namespace udet {

#define INST_PPT 16  // pixels per thread of the paint grid: 4096 pixels per workgroup amortise the flush of k partials
#define INST_K UDET_DET_MAX_K

__global__ __launch_bounds__(256) void inst_init_kernel(int n, const long long* __restrict__ offsets, const int* __restrict__ hw,
                                                        const long long* __restrict__ dets, const long long* __restrict__ counts, int k,
                                                        unsigned long long* __restrict__ row_gt,
                                                        unsigned long long* __restrict__ frame_stats, int* __restrict__ lookup) {
  const size_t stride = (size_t)gridDim.x * 256, g = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t j = g; j < (size_t)n * k; j += stride) {
    const int i = (int)(j / k), r = (int)(j - (size_t)i * k);
    row_gt[j] = 0;
    link_enter_roots(dets + (size_t)i * k * UDET_DET_FIELDS, link_rows(counts + 3 * i, k), (long long)hw[2 * i] * hw[2 * i + 1],
                     lookup + offsets[i], r);
  }
  for (size_t j = g; j < (size_t)3 * n; j += stride) frame_stats[j] = 0;
}

__global__ __launch_bounds__(256) void inst_paint_kernel(const int* __restrict__ labels, const long long* __restrict__ offsets,
                                                         const int* __restrict__ hw, const long long* __restrict__ dets,
                                                         const long long* __restrict__ counts, int k, const int* __restrict__ ids,
                                                         const unsigned char* __restrict__ gt, const int* __restrict__ lookup,
                                                         unsigned char* __restrict__ map, unsigned long long* __restrict__ row_gt,
                                                         unsigned long long* __restrict__ frame_stats) {
  __shared__ int root_s[INST_K], val_s[INST_K], part[INST_K], st[3];
  const int i = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int W = hw[2 * i + 1];
  const long long HW = (long long)hw[2 * i] * W, off = offsets[i];
  // the sample's pixels are walked from the aligned word its first byte lies in: pixel p sits at position p + a of that walk
  const int a = (int)((reinterpret_cast<uintptr_t>(map) + (unsigned long long)off) & 3);
  const long long span = HW + a;
  if ((long long)blockIdx.x * 256 >= span) return;  // beyond this sample's pixels (the whole workgroup)
  const int rows = link_rows(counts + 3 * i, k);
  for (int j = t; j < k; j += 256) {
    const long long root = j < rows ? dets[((size_t)i * k + j) * UDET_DET_FIELDS] : -1;
    const int id = j < rows ? ids[(size_t)i * k + j] : -1;
    root_s[j] = (root >= 0 && root < HW) ? (int)root : -1;
    val_s[j] = id >= 0 ? 1 + id % UDET_INSTANCE_WRAP : UDET_INSTANCE_UNASSIGNED;
    part[j] = 0;
  }
  if (t < 3) st[t] = 0;
  __syncthreads();
  const int* __restrict__ lab = labels + off;
  const int* __restrict__ look = lookup + off;
  const unsigned char* __restrict__ ann = gt ? gt + off : nullptr;
  unsigned char* __restrict__ mp = map + off;
  int n_assigned = 0, n_other = 0, n_gt = 0;  // of this wave
  for (long long base = (long long)blockIdx.x * 256; base < span; base += (long long)gridDim.x * 256) {  // block-uniform bounds
    const long long p = base + t - a;
    const bool valid = p >= 0 && p < HW;
    const int L = valid ? lab[p] : 0;
    const bool g = valid && ann && ann[p] != 0;
    int r = -1;
    unsigned v = 0;
    if (L >= 1 && L <= HW) {
      v = UDET_INSTANCE_UNASSIGNED;
      const int c = look[L - 1];  // never zeroed: only a rank whose row holds this root counts
      if ((unsigned)c < (unsigned)rows && root_s[c] == L - 1) { r = c; v = (unsigned)val_s[c]; }
    }
    const int hit = (r >= 0 && g) ? r : -1;
    const int len = det_run_length(hit, valid ? (int)(p % W) : 0, lane);
    if (len) atomicAdd(part + hit, len);  // a workgroup sees fewer than 2^31 pixels
    n_assigned += __popcll(__ballot(v >= 1 && v <= UDET_INSTANCE_WRAP));
    n_other += __popcll(__ballot(v == UDET_INSTANCE_UNASSIGNED));
    n_gt += __popcll(__ballot(g));
    store_packed_byte(mp, p, HW, lane, valid, v);  // aligned words of four pixels, the sample's head and tail byte by byte
  }
  if (lane == 0) {
    if (n_assigned) atomicAdd(st + 0, n_assigned);
    if (n_other) atomicAdd(st + 1, n_other);
    if (n_gt) atomicAdd(st + 2, n_gt);
  }
  __syncthreads();
  for (int j = t; j < k; j += 256)
    if (part[j]) atomicAdd(row_gt + (size_t)i * k + j, (unsigned long long)part[j]);
  if (t < 3 && st[t]) atomicAdd(frame_stats + (size_t)3 * i + t, (unsigned long long)st[t]);
}

// ---- udet_overlay_instances_ragged --------------------------------------------------------------------------------------------------
// The tile and the shifted groups of four pixels are overlay_native_kernel's (visualize.hip): a row's groups start where the element
// index offsets[i] + y W + x is a multiple of 4, so the tile's columns are [x0 - s, x0 + OI_TW - s) with s in 0..3 in that row.  V holds
// the map's bytes, column c = frame column x0 - OI_LEFT + c, row r = frame row y0 - edge + r, both clamped into the frame; Hmn / Hmx
// the minimum and maximum over x - edge .. x + edge, column hc = frame column x0 - 3 + hc.  The row strides are odd numbers of dwords.
#define OI_TH 32
#define OI_TW 64
#define OI_LEFT (3 + UDET_OVERLAY_MAX_EDGE)
#define OI_COLS (OI_TW + 3)                             // the columns x0 - 3 .. x0 + OI_TW - 1 a tile's groups can cover
#define OI_VW 84                                        // >= OI_LEFT + OI_TW + UDET_OVERLAY_MAX_EDGE, 21 dwords
#define OI_HW 68                                        // >= OI_COLS, 17 dwords
#define OI_ROWS (OI_TH + 2 * UDET_OVERLAY_MAX_EDGE)
static_assert(OI_LEFT + OI_TW + UDET_OVERLAY_MAX_EDGE <= OI_VW && OI_COLS <= OI_HW, "the tile and its halo fit their LDS rows");

__global__ __launch_bounds__(256) void overlay_instances_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ map,
                                                                const long long* __restrict__ offsets, const int* __restrict__ hw,
                                                                int tiles_x, float alpha, float beta, const unsigned* __restrict__ palette,
                                                                int palette_size, unsigned other_rgb, int edge,
                                                                unsigned char* __restrict__ out, int wide) {
  __shared__ unsigned char V[OI_ROWS][OI_VW];
  __shared__ unsigned char Hmn[OI_ROWS][OI_HW], Hmx[OI_ROWS][OI_HW];
  __shared__ unsigned pal[UDET_TRACK_MAX_PALETTE];
  const int n = blockIdx.y, t = threadIdx.x;
  const int H = hw[2 * n], W = hw[2 * n + 1];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * OI_TH, x0 = tx * OI_TW;
  if (y0 >= H || x0 - 3 >= W) return;  // beyond this sample's tiles (the whole workgroup: nothing below is reached)
  const long off = offsets[n];
  const int rows = OI_TH + 2 * edge;

  // 1. the bytes a contour of this tile can depend on: columns x0 - 3 - edge .. x0 + OI_TW - 1 + edge of the rows y0 - edge .. y0 + OI_TH
  // - 1 + edge, each coordinate clamped into the frame (edge = 0: the tile's own pixels)
  for (int j = t; j < palette_size; j += 256) pal[j] = palette[j] & 0xffffffu;
  const int c_lo = OI_LEFT - 3 - edge, cw = OI_COLS + 2 * edge;
  for (int it = t; it < rows * cw; it += 256) {
    const int r = it / cw, c = c_lo + (it - r * cw);
    const int gy = min(max(y0 - edge + r, 0), H - 1), gx = min(max(x0 - OI_LEFT + c, 0), W - 1);
    V[r][c] = map[off + (long)gy * W + gx];
  }
  __syncthreads();

  // 2. the windowed minimum and maximum along the rows
  if (edge > 0) {
    for (int it = t; it < rows * OI_COLS; it += 256) {
      const int r = it / OI_COLS, hc = it - r * OI_COLS;
      const unsigned char* __restrict__ v = &V[r][hc + OI_LEFT - 3];
      unsigned mn = 255u, mx = 0u;
      for (int d = -edge; d <= edge; ++d) {
        const unsigned u = v[d];
        mn = min(mn, u);
        mx = max(mx, u);
      }
      Hmn[r][hc] = (unsigned char)mn;
      Hmx[r][hc] = (unsigned char)mx;
    }
    __syncthreads();
  }

  // 3. along the columns, blend and contour: two groups of four pixels per thread, 16 groups (192 contiguous bytes) per row
  const unsigned other = other_rgb & 0xffffffu;
  const int k = t & 15;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int ry = (t >> 4) + 16 * half, gy = y0 + ry;
    if (gy >= H) continue;
    const long b = off + (long)gy * W;  // element index of the row's first pixel
    const int s = (int)(b & 3);
    const int xf = x0 - s + 4 * k;      // the group's first pixel: b + xf is a multiple of 4
    if (xf + 3 < 0 || xf >= W) continue;
    const int hc0 = 3 - s + 4 * k;
    unsigned col[4], ct = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned v = V[ry + edge][hc0 + j + OI_LEFT - 3];
      col[j] = v == 0u ? 0u : (v <= UDET_INSTANCE_WRAP ? pal[(v - 1u) % (unsigned)palette_size] : other);
      if (edge > 0 && v != 0u) {
        unsigned mn = 255u, mx = 0u;
        for (int r = ry; r <= ry + 2 * edge; ++r) {
          mn = min(mn, (unsigned)Hmn[r][hc0 + j]);
          mx = max(mx, (unsigned)Hmx[r][hc0 + j]);
        }
        if (mn != v || mx != v) ct |= 1u << j;
      }
    }
    rgb_group4(image, out, b, xf, W, wide, [&](int j, int c, unsigned v) -> unsigned {
      const unsigned m = (col[j] >> (16 - 8 * c)) & 255u;  // 0 on background: the blend's second term is then + 0
      return ((ct >> j) & 1u) ? m : native_blend(v, alpha, (float)m * beta);
    });
  }
}

}  // namespace udet

using namespace udet;

extern "C" {

size_t udet_track_instance_maps_workspace_bytes(size_t total_pixels, int n, int k) {
  if (n < 1 || n > 65535 || total_pixels < 1 || k < 1 || k > UDET_DET_MAX_K) return 0;
  return total_pixels * sizeof(int);  // the root-to-rank lookup; no per-sample term
}

int udet_track_instance_maps_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                    size_t total_pixels, const long long* dets, const long long* counts, int k, const int* ids,
                                    const unsigned char* gt, unsigned char* map, long long* row_gt, long long* frame_stats,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch("track_instance_maps_ragged", n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (!labels || !offsets || !hw || !dets || !counts || !ids || !map || !row_gt || !frame_stats) {
    set_error("track_instance_maps_ragged: bad argument (non-null labels, offsets, hw, dets, counts, ids, map, row_gt and frame_stats)");
    return UDET_ERR_ARG;
  }
  if (k < 1 || k > UDET_DET_MAX_K) {
    set_error("track_instance_maps_ragged: k = %d in 1..UDET_DET_MAX_K = %d is required", k, UDET_DET_MAX_K);
    return UDET_ERR_ARG;
  }
  if (bad_workspace("track_instance_maps_ragged", workspace, workspace_bytes, udet_track_instance_maps_workspace_bytes(total_pixels, n, k), 4))
    return UDET_ERR_ARG;
  const uintptr_t a4 = reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(ids);
  const uintptr_t a8 = reinterpret_cast<uintptr_t>(dets) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(row_gt) |
                       reinterpret_cast<uintptr_t>(frame_stats);
  if ((a4 & 3) || (a8 & 7)) {
    set_error("track_instance_maps_ragged: labels and ids must be 4-byte aligned, dets, counts, row_gt and frame_stats 8-byte aligned");
    return UDET_ERR_ARG;
  }
  const long nb = ((long)max_h * max_w + 3 + 256 * INST_PPT - 1) / (256 * INST_PPT);  // + 3: the walk starts at an aligned word
  const size_t nz = ((size_t)n * k + 255) / 256;
  int* lookup = (int*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(inst_init_kernel, dim3((unsigned)(nz > 65536 ? 65536 : nz)), dim3(256), 0, s, n, offsets, hw, dets, counts, k,
                     (unsigned long long*)row_gt, (unsigned long long*)frame_stats, lookup);
  hipLaunchKernelGGL(inst_paint_kernel, dim3((unsigned)nb, n), dim3(256), 0, s, labels, offsets, hw, dets, counts, k, ids, gt, lookup, map,
                     (unsigned long long*)row_gt, (unsigned long long*)frame_stats);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

int udet_overlay_instances_ragged(const unsigned char* image_rgb, const unsigned char* map, int n, const long long* offsets, const int* hw,
                                  int max_h, int max_w, size_t total_pixels, float alpha, float beta, const unsigned* palette,
                                  int palette_size, unsigned other_rgb, int edge, unsigned char* out_rgb, void* stream) {
  if (bad_batch("overlay_instances_ragged", n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (!image_rgb || !map || !offsets || !hw || !palette || !out_rgb) {
    set_error("overlay_instances_ragged: bad argument (non-null image_rgb, map, offsets, hw, palette and out_rgb)");
    return UDET_ERR_ARG;
  }
  if (edge < 0 || !(alpha >= 0.f) || !(beta >= 0.f) || isinf(alpha) || isinf(beta)) {
    set_error("overlay_instances_ragged: edge %d >= 0 and finite alpha %g >= 0 and beta %g >= 0 are required", edge, alpha, beta);
    return UDET_ERR_ARG;
  }
  if (palette_size < 1 || palette_size > UDET_TRACK_MAX_PALETTE || (reinterpret_cast<uintptr_t>(palette) & 3) || other_rgb > 0xffffffu) {
    set_error("overlay_instances_ragged: a 4-byte aligned palette of %d in 1..%d colours and other_rgb = 0x%x of 24 bits are required",
              palette_size, UDET_TRACK_MAX_PALETTE, other_rgb);
    return UDET_ERR_ARG;
  }
  if (edge > UDET_OVERLAY_MAX_EDGE) {
    set_error("overlay_instances_ragged: edge %d above UDET_OVERLAY_MAX_EDGE = %d", edge, UDET_OVERLAY_MAX_EDGE);
    return UDET_ERR_UNSUPPORTED;
  }
  // a row's groups of four pixels start up to three columns before the tile's first: ceil((max_w + 3) / OI_TW) tile columns
  const long tiles_x = ((long)max_w + 3 + OI_TW - 1) / OI_TW, tiles_y = ((long)max_h + OI_TH - 1) / OI_TH;
  if (tiles_x * tiles_y > (1L << 23)) {
    set_error("overlay_instances_ragged: more than 2^23 tiles per sample");
    return UDET_ERR_SHAPE;
  }
  const int wide = ((reinterpret_cast<uintptr_t>(image_rgb) | reinterpret_cast<uintptr_t>(out_rgb)) & 3) == 0;
  hipLaunchKernelGGL(overlay_instances_kernel, dim3((unsigned)(tiles_x * tiles_y), n), dim3(256), 0, (hipStream_t)stream, image_rgb, map,
                     offsets, hw, (int)tiles_x, alpha, beta, palette, palette_size, other_rgb, edge, out_rgb, wide);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // extern "C"
