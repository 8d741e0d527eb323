// DAVIS contour accuracy on the GPU: the four integers per frame behind the boundary F-measure.
// A restatement of the published DAVIS measure db_eval_boundary (Perazzi et al., CVPR 2016; the benchmark's Python toolkit, which --
// like skimage and cv2 -- is not part of this project): the reference tree has no code for it.  Definitions: include/udet.h,
// udet_boundary_stats; DESIGN.md "DAVIS metrics".
//
// Everything is integer and bit-packed.  One workgroup owns a tile of TH rows x 256 columns of one sample:
//   1. the thresholded (and, for the prediction, possibly complemented) masks of the tile plus a halo of r rows (and one more row below)
//      and one 64-column word left and right are packed into LDS, one __ballot per (row, word): bit l of word j is column 64 j + l;
//   2. the boundary words of both masks follow from word-wide XORs of a row, its successor and their one-bit shifts;
//   3. a wave takes one (row, word) of the tile's core with at least one boundary pixel, one pixel per lane, and walks the rows
//      y, y-1, y+1, ... y-r, y+r of the OTHER mask's boundary: the pixel matches when row_bits & window(x - wx(dy), x + wx(dy)) is non-zero,
//      wx(dy) = floor(sqrt(r^2 - dy^2)) the half-width of the disk at that row offset.  A window of at most 127 bits touches the pixel's own
//      word and its two neighbours; every lane reads the same three words (LDS broadcast).  The walk ends as soon as every boundary
//      pixel of the word has matched.
// Counts are accumulated per wave and added with one 64-bit integer atomicAdd per counter: exact, independent of the order.
#include "common.h"
#include "elementwise.h"

namespace udet {

#define BS_WORDS 4              // 64-column words of a tile's core
#define BS_NW (BS_WORDS + 2)    // + one halo word on each side: covers every radius <= UDET_BOUNDARY_MAX_RADIUS = 63
static_assert(UDET_BOUNDARY_MAX_RADIUS <= 63, "one halo word per side");

__host__ __device__ inline int boundary_tile_rows(int r) { return r <= 16 ? 32 : 64; }
// LDS: packed masks (TH + 2r + 1 rows) and boundary maps (TH + 2r rows) of both inputs, the disk's half-widths
static size_t boundary_lds_bytes(int r) {
  const int th = boundary_tile_rows(r);
  return (size_t)8 * BS_NW * (2 * (th + 2 * r + 1) + 2 * (th + 2 * r)) + 64 * sizeof(int);
}

__global__ __launch_bounds__(256) void boundary_stats_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             const double* __restrict__ stats8, int H, int W, float threshold,
                                                             float gt_threshold, int r, int tiles_x,
                                                             unsigned long long* __restrict__ counts4,
                                                             unsigned char* __restrict__ bmap_pred, unsigned char* __restrict__ bmap_gt) {
  extern __shared__ unsigned long long lds[];
  const int TH = boundary_tile_rows(r);
  const int RS = TH + 2 * r + 1, RB = TH + 2 * r;
  unsigned long long* const Sp = lds;               // [RS][BS_NW] packed prediction, row 0 = image row y0 - r, word 0 = image word j0 - 1
  unsigned long long* const Sg = Sp + RS * BS_NW;   // [RS][BS_NW] packed ground truth
  unsigned long long* const Bp = Sg + RS * BS_NW;   // [RB][BS_NW] boundary of the prediction
  unsigned long long* const Bg = Bp + RB * BS_NW;   // [RB][BS_NW] boundary of the ground truth
  int* const wxs = reinterpret_cast<int*>(Bg + RB * BS_NW);  // [r + 1] half-width of the disk at row offset dy

  const int n = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * TH, j0 = tx * BS_WORDS;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long base = (long)n * H * W;
  // disambiguate_forw_back (general_utils.py:100-109), the expression udet_flow_to_image / udet_overlay_mask use
  const bool flip = stats8 && stats8[(long)n * 8] / (4.0 * W + 4.0 * H) >= 0.6;

  if ((int)threadIdx.x <= r) {  // floor(sqrt(r^2 - dy^2)), exact: the float root is corrected in integers
    const int v = r * r - (int)threadIdx.x * (int)threadIdx.x;
    int s = (int)sqrtf((float)v);
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    wxs[threadIdx.x] = s;
  }

  // 1. pack: one (row, word) per wave and iteration, one coalesced 256-byte row segment of each mask
  for (int it = wave; it < RS * BS_NW; it += 4) {
    const int row = it / BS_NW, word = it - row * BS_NW;
    const int gy = y0 - r + row, gx0 = (j0 - 1 + word) * 64;
    unsigned long long sp = 0, sg = 0;
    if (gy >= 0 && gy < H && gx0 >= 0 && gx0 < W) {  // wave-uniform
      const int gx = gx0 + lane;
      const long q = base + (long)gy * W + min(gx, W - 1);
      const float pv = pred[q], gv = gt[q];
      sp = __ballot(gx < W && ((pv > threshold) != flip));
      sg = __ballot(gx < W && gv > gt_threshold);
    }
    if (lane == 0) {
      Sp[it] = sp;
      Sg[it] = sg;
    }
  }
  __syncthreads();

  // 2. boundary words (udet.h, definition 1).  The successor of the last halo word is not loaded and taken as zero: only bit 63 of the
  // right halo word depends on it, and a window reaches at most 63 columns past the core.
  for (int it = threadIdx.x; it < RB * BS_NW; it += 256) {
    const int row = it / BS_NW, word = it - row * BS_NW;
    const int gy = y0 - r + row, j = j0 - 1 + word;
    unsigned long long bp = 0, bg = 0;
    if (gy >= 0 && gy < H && j >= 0 && j * 64 < W) {
      const int left = W - j * 64;  // columns of the image from this word's first
      const unsigned long long valid = left >= 64 ? ~0ull : (1ull << left) - 1;
      const unsigned long long lastcol = left <= 64 ? 1ull << (left - 1) : 0ull;
      const bool more = word + 1 < BS_NW;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const unsigned long long* S = m ? Sg : Sp;
        const unsigned long long c = S[it], cn = more ? S[it + 1] : 0ull;
        const unsigned long long e = (c >> 1) | (cn << 63);
        unsigned long long b;
        if (gy == H - 1) {
          b = (c ^ e) & valid & ~lastcol;  // last row: seg ^ e, the corner 0
        } else {
          const unsigned long long s = S[it + BS_NW], sn = more ? S[it + BS_NW + 1] : 0ull;
          const unsigned long long se = (s >> 1) | (sn << 63);
          b = (((c ^ e) | (c ^ s) | (c ^ se)) & valid & ~lastcol) | ((c ^ s) & lastcol);  // last column: seg ^ s
        }
        if (m) bg = b; else bp = b;
      }
    }
    Bp[it] = bp;
    Bg[it] = bg;
  }
  __syncthreads();

  // 3. count and match.  Item = (direction, core row, core word); direction 0 searches the prediction's boundary pixels in the ground
  // truth's boundary, direction 1 the reverse.  cnt / hit hold the same value in every lane (ballots).
  unsigned cnt[2] = {0, 0}, hit[2] = {0, 0};
  for (int it = wave; it < 2 * TH * BS_WORDS; it += 4) {
    const int dir = it / (TH * BS_WORDS), rem = it - dir * (TH * BS_WORDS);
    const int yy = rem / BS_WORDS, jj = rem - yy * BS_WORDS;
    const unsigned long long* A = dir ? Bg : Bp;
    const unsigned long long* T = dir ? Bp : Bg;
    const int centre = (yy + r) * BS_NW + jj + 1;
    const bool mine = (A[centre] >> lane) & 1ull;
    unsigned char* bm = dir ? bmap_gt : bmap_pred;
    if (bm) {
      const int gy = y0 + yy, gx = (j0 + jj) * 64 + lane;
      if (gy < H && gx < W) bm[base + (long)gy * W + gx] = mine ? 1 : 0;
    }
    const unsigned long long act = __ballot(mine);
    if (act == 0) continue;
    bool pending = mine;
    for (int d = 0; d <= r; ++d) {
      const int wx = wxs[d];
      const int lo = lane - wx, hi = lane + wx;  // window in columns relative to the pixel's own word
      const unsigned long long mC = (~0ull >> (63 - min(hi, 63))) & (~0ull << max(lo, 0));
      const unsigned long long mL = lo < 0 ? ~0ull << (64 + lo) : 0ull;
      const unsigned long long mR = hi > 63 ? ~0ull >> (127 - hi) : 0ull;
      const unsigned long long* up = T + centre - d * BS_NW;
      const unsigned long long* dn = T + centre + d * BS_NW;
      const unsigned long long f = ((up[-1] | dn[-1]) & mL) | ((up[0] | dn[0]) & mC) | ((up[1] | dn[1]) & mR);
      pending = pending && f == 0;
      if (__ballot(pending) == 0) break;
    }
    const unsigned long long matched = __ballot(mine && !pending);
    if (dir) {
      cnt[1] += __popcll(act);
      hit[1] += __popcll(matched);
    } else {
      cnt[0] += __popcll(act);
      hit[0] += __popcll(matched);
    }
  }
  if (lane == 0) {
    unsigned long long* o = counts4 + (long)n * 4;
    if (cnt[0]) atomicAdd(o + 0, (unsigned long long)cnt[0]);
    if (cnt[1]) atomicAdd(o + 1, (unsigned long long)cnt[1]);
    if (hit[0]) atomicAdd(o + 2, (unsigned long long)hit[0]);
    if (hit[1]) atomicAdd(o + 3, (unsigned long long)hit[1]);
  }
}

int launch_boundary_stats(const float* pred, const float* gt, const double* stats8, int N, int H, int W, float threshold,
                          float gt_threshold, int radius, unsigned long long* counts4, unsigned char* bmap_pred,
                          unsigned char* bmap_gt, hipStream_t s) {
  const int th = boundary_tile_rows(radius);
  const long tiles_x = ((long)W + 64 * BS_WORDS - 1) / (64 * BS_WORDS), tiles_y = ((long)H + th - 1) / th;
  if (tiles_x * tiles_y > 0x7fffffffL) { set_error("boundary_stats: image too large"); return UDET_ERR_SHAPE; }
  UDET_HIP(hipMemsetAsync(counts4, 0, (size_t)N * 4 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(boundary_stats_kernel, dim3((unsigned)(tiles_x * tiles_y), N), dim3(256), boundary_lds_bytes(radius), s, pred, gt,
                     stats8, H, W, threshold, gt_threshold, radius, (int)tiles_x, counts4, bmap_pred, bmap_gt);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
