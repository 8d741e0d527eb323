// Connected components of a ragged batch of binary masks and the choice of one of them per sample: the "best
// detection candidate from the set of predicted connected masks" of post_processing/post_processing.py:32-35, for which the reference
// has a comment and no code.  Input: the packed layout restore.hip writes (sample i = H_i x W_i bytes at offsets[i]).  A component's
// root is the smallest row-major index y * W + x among its pixels; a foreground pixel's label is root + 1, background 0.  Five
// launches however many samples there are, all on many workgroups per sample, none of which waits for another:
//   1. components_tile_kernel     one 64 x 32 tile of one sample per workgroup: union-find in LDS (atomicMin on the parent, the larger
//                                 root always linked under the smaller), each pixel's label = the global index of its tile root + 1;
//                                 zeroes the per-pixel area / inter counters and the sample's annotation count
//   2. components_border_kernel   the pixels on a tile's top row and left / right column union with their W / N (NW / NE) neighbours
//                                 in the adjacent tiles -- across tile corners too -- in global memory: agent-scope loads + atomicMin
//   3. components_flatten_kernel  label = root + 1 for every pixel; area / inter of the root accumulated with one integer atomic per
//                                 horizontal run of a wave (a run lies in one component); |gt| of the sample
//   4. components_partial_kernel  per sample COMPONENTS_NB workgroups: the number of roots and the best root of a strided share
//   5. components_select_kernel   every wave reduces the sample's partial winners (one per lane, shuffles), writes its share of
//                                 `selected`; info
// Every walk over parents moves to strictly smaller indices (label <= own index + 1 always), so every loop ends, and the final
// forest -- each pixel under the smallest index of its component -- does not depend on the order the workgroups ran in.  Integer
// work only: the outputs are exact and identical from run to run.  Every index comes from offsets / hw, which the caller validates on
// the host (native_results.check_component_tables).
#include "common.h"
#include "elementwise.h"

namespace udet {

#define COMPONENTS_TW 64   // tile: 64 columns (one lane per column)
#define COMPONENTS_TH 32   //       x 32 rows, eight per thread           (UDET_COMPONENTS_TILE_W / _H of include/udet.h)
#define COMPONENTS_NB 32   // partial winners per sample (at most 64: one per lane in the final reduce)
#define COMPONENTS_PPT 8   // pixels per thread of the flatten / select grids

static_assert(COMPONENTS_TW == UDET_COMPONENTS_TILE_W && COMPONENTS_TH == UDET_COMPONENTS_TILE_H, "tile size of include/udet.h");

// ---- union-find on an int array of labels (parent + 1; 0 = background) shared with other threads --------------------------------
// LDS flavour (workgroup scope) for the tile, global flavour (agent scope: another XCD's atomics are seen) for the border pass.
template <bool GLOBAL>
__device__ __forceinline__ int cc_load(const int* p) {
  return GLOBAL ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GLOBAL>
__device__ __forceinline__ int cc_find(const int* lab, int x) {
  int v;
  while ((v = cc_load<GLOBAL>(lab + x) - 1) != x) x = v;  // v < x
  return x;
}
template <bool GLOBAL>
__device__ __forceinline__ void cc_union(int* lab, int a, int b) {
  for (;;) {
    a = cc_find<GLOBAL>(lab, a);
    b = cc_find<GLOBAL>(lab, b);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(lab + a, b + 1) - 1;  // a > b: link a under b if a is still a root
    if (old == a) return;
    a = old;  // old < a: a had been linked meanwhile; go on from there (the link a -> old, if just replaced, is re-made by this walk)
  }
}

__global__ __launch_bounds__(256) void components_tile_kernel(const unsigned char* __restrict__ binary, const long long* __restrict__ offsets,
                                                              const int* __restrict__ hw, int conn8, int* __restrict__ labels,
                                                              int* __restrict__ area, int* __restrict__ inter, int* __restrict__ gsum) {
  __shared__ int lab[COMPONENTS_TW * COMPONENTS_TH];
  const int i = blockIdx.y, t = threadIdx.x;
  const int H = hw[2 * i], W = hw[2 * i + 1];
  const int tiles_x = (W + COMPONENTS_TW - 1) / COMPONENTS_TW, tiles_y = (H + COMPONENTS_TH - 1) / COMPONENTS_TH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // block-uniform: the grid is sized for the largest frame of the batch
  if (blockIdx.x == 0 && t == 0) gsum[i] = 0;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int lx = t & (COMPONENTS_TW - 1), X = tx * COMPONENTS_TW + lx, Y0 = ty * COMPONENTS_TH;
  const size_t o = (size_t)offsets[i];
  const unsigned char* __restrict__ b = binary + o;
  for (int ly = t >> 6; ly < COMPONENTS_TH; ly += 4) {
    const int Y = Y0 + ly, l = ly * COMPONENTS_TW + lx;
    lab[l] = (X < W && Y < H && b[(size_t)Y * W + X] != 0) ? l + 1 : 0;
  }
  __syncthreads();
  for (int ly = t >> 6; ly < COMPONENTS_TH; ly += 4) {
    const int l = ly * COMPONENTS_TW + lx;
    if (cc_load<false>(lab + l) == 0) continue;  // a label never becomes 0 or leaves 0
    const bool w = lx > 0 && cc_load<false>(lab + l - 1) != 0;
    if (w) cc_union<false>(lab, l, l - 1);
    if (ly == 0) continue;
    if (cc_load<false>(lab + l - COMPONENTS_TW) != 0) {
      cc_union<false>(lab, l, l - COMPONENTS_TW);  // N joins NW and NE itself (its own W, and NE's W)
    } else if (conn8) {
      if (!w && lx > 0 && cc_load<false>(lab + l - COMPONENTS_TW - 1) != 0) cc_union<false>(lab, l, l - COMPONENTS_TW - 1);  // else W's N
      if (lx < COMPONENTS_TW - 1 && cc_load<false>(lab + l - COMPONENTS_TW + 1) != 0) cc_union<false>(lab, l, l - COMPONENTS_TW + 1);
    }
  }
  __syncthreads();
  for (int ly = t >> 6; ly < COMPONENTS_TH; ly += 4) {
    const int Y = Y0 + ly, l = ly * COMPONENTS_TW + lx;
    if (X >= W || Y >= H) continue;
    int v = 0;
    if (lab[l] != 0) {
      const int r = cc_find<false>(lab, l);  // the tile's smallest local index = its smallest row-major index in the frame
      v = (Y0 + (r >> 6)) * W + tx * COMPONENTS_TW + (r & (COMPONENTS_TW - 1)) + 1;
    }
    const size_t k = o + (size_t)Y * W + X;
    labels[k] = v;
    area[k] = 0;
    inter[k] = 0;
  }
}

__global__ __launch_bounds__(256) void components_border_kernel(const unsigned char* __restrict__ binary, const long long* __restrict__ offsets,
                                                                const int* __restrict__ hw, int conn8, int* labels) {
  const int i = blockIdx.y, t = threadIdx.x;
  const int H = hw[2 * i], W = hw[2 * i + 1];
  const int tiles_x = (W + COMPONENTS_TW - 1) / COMPONENTS_TW, tiles_y = (H + COMPONENTS_TH - 1) / COMPONENTS_TH;
  if ((int)blockIdx.x >= tiles_x * tiles_y || t >= COMPONENTS_TW + 2 * COMPONENTS_TH) return;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = tx * COMPONENTS_TW, Y0 = ty * COMPONENTS_TH;
  const size_t o = (size_t)offsets[i];
  const unsigned char* __restrict__ b = binary + o;
  int* lab = labels + o;
  // the neighbours W, N, NW, NE of (X, Y) that lie in another tile; each adjacent pair of the frame is met from its later pixel
  int X, Y;
  bool w = false, n = false, nw = false, ne = false;
  if (t < COMPONENTS_TW) {  // top row: N, NW, NE in the tiles above (NW of the first and NE of the last column: across the corner)
    X = X0 + t; Y = Y0;
    n = Y > 0;
    nw = conn8 && Y > 0 && X > 0;
    ne = conn8 && Y > 0 && X + 1 < W;
  } else if (t < COMPONENTS_TW + COMPONENTS_TH) {  // left column: W, and NW below the top row, in the tile to the left
    X = X0; Y = Y0 + t - COMPONENTS_TW;
    w = X > 0;
    nw = conn8 && X > 0 && Y > Y0;
  } else {  // right column below the top row: NE in the tile to the right
    X = X0 + COMPONENTS_TW - 1; Y = Y0 + t - COMPONENTS_TW - COMPONENTS_TH;
    ne = conn8 && Y > Y0 && X + 1 < W;
  }
  if (X >= W || Y >= H) return;
  const int k = Y * W + X;
  if (b[k] == 0) return;
  if (w && b[k - 1] != 0) cc_union<true>(lab, k, k - 1);
  if (n && b[k - W] != 0) cc_union<true>(lab, k, k - W);
  if (nw && b[k - W - 1] != 0) cc_union<true>(lab, k, k - W - 1);
  if (ne && b[k - W + 1] != 0) cc_union<true>(lab, k, k - W + 1);
}

__global__ __launch_bounds__(256) void components_flatten_kernel(int* labels, const unsigned char* __restrict__ gt,
                                                                 const long long* __restrict__ offsets, const int* __restrict__ hw,
                                                                 int* __restrict__ area, int* __restrict__ inter, int* __restrict__ gsum) {
  const int i = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int W = hw[2 * i + 1];
  const long long HW = (long long)hw[2 * i] * W;
  const size_t o = (size_t)offsets[i];
  int* lab = labels + o;
  int gcount = 0;
  for (long long base = (long long)blockIdx.x * 256; base < HW; base += (long long)gridDim.x * 256) {  // block-uniform bounds
    const long long k = base + t;
    const bool valid = k < HW;
    int r = -1;
    // Every label this kernel stores is the root its reader would reach anyway: whichever of the two a walk meets, it ends at the root.
    if (valid && lab[k] != 0) {
      r = cc_find<true>(lab, lab[k] - 1);
      lab[k] = r + 1;
    }
    const int x = valid ? (int)k % W : 0;
    const bool fg = r >= 0, g = valid && gt && gt[o + k] != 0;
    const unsigned long long mfg = __ballot(fg), mcont = __ballot(fg && x != 0), mg = __ballot(g);
    gcount += __popcll(mg);
    // a horizontal run of foreground lanes lies in one component: its first lane adds the run's length (and its annotated pixels)
    if (fg && (lane == 0 || x == 0 || !((mfg >> (lane - 1)) & 1))) {
      const unsigned long long rest = lane == 63 ? 0ull : (mcont >> (lane + 1));  // the top bit of rest is 0: ~rest is never 0
      const int len = __ffsll((long long)~rest);                                // 1 + the lanes after this one that continue the run
      const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1)) << lane;
      const int ni = __popcll(mg & run);
      atomicAdd(area + o + r, len);
      if (ni) atomicAdd(inter + o + r, ni);
    }
  }
  if (lane == 0 && gcount) atomicAdd(gsum + i, gcount);
}

// a = (root, area, inter) is the better candidate of the two; root < 0: no candidate.  G = |gt| of the sample.
__device__ __forceinline__ bool cc_better(int mode, int a_root, int a_area, int a_inter, int b_root, int b_area, int b_inter, int G) {
  if (a_root < 0) return false;
  if (b_root < 0) return true;
  if (mode == UDET_COMPONENTS_BEST_GT) {  // inter / (area + G - inter), compared by cross-multiplication: every product < 2^63
    const unsigned long long l = (unsigned long long)a_inter * ((unsigned long long)b_area + G - b_inter);
    const unsigned long long r = (unsigned long long)b_inter * ((unsigned long long)a_area + G - a_inter);
    if (l != r) return l > r;
  }
  if (a_area != b_area) return a_area > b_area;
  return a_root < b_root;
}

__global__ __launch_bounds__(256) void components_partial_kernel(const int* __restrict__ labels, const long long* __restrict__ offsets,
                                                                 const int* __restrict__ hw, const int* __restrict__ area,
                                                                 const int* __restrict__ inter, const int* __restrict__ gsum, int mode,
                                                                 long long* __restrict__ part) {
  __shared__ int sroot[256], sarea[256], sinter[256], scount[256];
  const int i = blockIdx.y, t = threadIdx.x;
  const long long HW = (long long)hw[2 * i] * hw[2 * i + 1];
  const size_t o = (size_t)offsets[i];
  const int G = gsum[i];
  int root = -1, ar = 0, in = 0, count = 0;
  for (long long k = (long long)blockIdx.x * 256 + t; k < HW; k += COMPONENTS_NB * 256) {
    if (labels[o + k] != (int)k + 1) continue;
    ++count;
    const int a = area[o + k], b = inter[o + k];
    if (cc_better(mode, (int)k, a, b, root, ar, in, G)) { root = (int)k; ar = a; in = b; }
  }
  sroot[t] = root; sarea[t] = ar; sinter[t] = in; scount[t] = count;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      scount[t] += scount[t + s];
      if (cc_better(mode, sroot[t + s], sarea[t + s], sinter[t + s], sroot[t], sarea[t], sinter[t], G)) {
        sroot[t] = sroot[t + s]; sarea[t] = sarea[t + s]; sinter[t] = sinter[t + s];
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    long long* __restrict__ p = part + ((size_t)i * COMPONENTS_NB + blockIdx.x) * 4;
    p[0] = scount[0]; p[1] = sroot[0]; p[2] = sarea[0]; p[3] = sinter[0];
  }
}

__global__ __launch_bounds__(256) void components_select_kernel(const int* __restrict__ labels, const long long* __restrict__ offsets,
                                                                const int* __restrict__ hw, const int* __restrict__ gsum,
                                                                const long long* __restrict__ part, int mode,
                                                                unsigned char* __restrict__ selected, long long* __restrict__ info) {
  const int i = blockIdx.y, t = threadIdx.x;
  const long long HW = (long long)hw[2 * i] * hw[2 * i + 1];
  const size_t o = (size_t)offsets[i];
  const int G = gsum[i];
  // the partial winners of launch 4: one per lane, then a butterfly over the wave -- the order is total (roots are distinct), so every
  // lane of every wave ends with the same winner and the same count
  // (Written as a uniform loop over the 32 partials this compiled, at -O3 for gfx950, to scalar code that kept the previous winner's
  // inter when a later partial won on area or root; tests/test_components_gpu.py compares every info entry.)
  int count = 0, root = -1, ar = 0, in = 0;
  if ((t & 63) < COMPONENTS_NB) {
    const long long* p = part + ((size_t)i * COMPONENTS_NB + (t & 63)) * 4;
    count = (int)p[0]; root = (int)p[1]; ar = (int)p[2]; in = (int)p[3];
  }
  for (int s = 32; s > 0; s >>= 1) {
    const int oc = __shfl_xor(count, s), orr = __shfl_xor(root, s), oa = __shfl_xor(ar, s), oi = __shfl_xor(in, s);
    count += oc;
    if (cc_better(mode, orr, oa, oi, root, ar, in, G)) { root = orr; ar = oa; in = oi; }
  }
  if (mode == UDET_COMPONENTS_LABEL) { root = -1; ar = 0; in = 0; }
  if (blockIdx.x == 0 && t == 0) {
    info[4 * i] = count; info[4 * i + 1] = root; info[4 * i + 2] = ar; info[4 * i + 3] = in;
  }
  if (!selected) return;
  for (long long k = (long long)blockIdx.x * 256 + t; k < HW; k += (long long)gridDim.x * 256)
    selected[o + k] = (root >= 0 && labels[o + k] == root + 1) ? 1 : 0;
}

// workspace: partial winners (int64), then per-sample |gt|, then labels / area / inter (int32 per pixel of the packed buffer)
static inline size_t cc_part_bytes(int n) { return (size_t)n * COMPONENTS_NB * 4 * sizeof(long long); }
static inline size_t cc_gsum_bytes(int n) { return (((size_t)n + 1) & ~(size_t)1) * sizeof(int); }
size_t components_workspace_bytes(size_t total_pixels, int n) { return cc_part_bytes(n) + cc_gsum_bytes(n) + 3 * total_pixels * sizeof(int); }

int launch_select_components_ragged(const unsigned char* binary, const unsigned char* gt, int n, const long long* offsets, const int* hw,
                                    int max_h, int max_w, size_t total_pixels, int connectivity, int mode, int* labels,
                                    unsigned char* selected, long long* info, void* workspace, hipStream_t s) {
  const long tiles = (long)((max_w + COMPONENTS_TW - 1) / COMPONENTS_TW) * ((max_h + COMPONENTS_TH - 1) / COMPONENTS_TH);
  const long nb = ((long)max_h * max_w + 256 * COMPONENTS_PPT - 1) / (256 * COMPONENTS_PPT);
  if (tiles > 0x7fffffffL || nb > 0x7fffffffL) { set_error("select_components_ragged: frame too large"); return UDET_ERR_SHAPE; }
  char* ws = (char*)workspace;
  long long* part = (long long*)ws;
  int* gsum = (int*)(ws + cc_part_bytes(n));
  int* own = (int*)(ws + cc_part_bytes(n) + cc_gsum_bytes(n));
  int* lab = labels ? labels : own;
  int* area = own + total_pixels;
  int* inter = area + total_pixels;
  const int conn8 = connectivity == 8;
  hipLaunchKernelGGL(components_tile_kernel, dim3((unsigned)tiles, n), dim3(256), 0, s, binary, offsets, hw, conn8, lab, area, inter, gsum);
  hipLaunchKernelGGL(components_border_kernel, dim3((unsigned)tiles, n), dim3(256), 0, s, binary, offsets, hw, conn8, lab);
  hipLaunchKernelGGL(components_flatten_kernel, dim3((unsigned)nb, n), dim3(256), 0, s, lab, gt, offsets, hw, area, inter, gsum);
  hipLaunchKernelGGL(components_partial_kernel, dim3(COMPONENTS_NB, n), dim3(256), 0, s, lab, offsets, hw, area, inter, gsum, mode, part);
  hipLaunchKernelGGL(components_select_kernel, dim3(selected ? (unsigned)nb : 1u, n), dim3(256), 0, s, lab, offsets, hw, gsum, part, mode,
                     selected, info);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // namespace udet
