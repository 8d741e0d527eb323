// Tracks against multi-object annotations, from what the link left on the device: udet_track_object_overlaps_ragged
// counts for n frames (packed layout, sample i = H_i x W_i at offsets[i]) the pixels every row shares with every annotated object, every
// object's own pixels and two counts per frame.  objects is a byte per pixel: 0 background, 1..O an annotated object, above O "void".
//   1. obj_init_kernel            zeroes row_obj, obj_area and frame_stats and writes every row's rank at its root into the workspace -- the
//                                 lookup of the link (track_rows.h): one int32 per pixel, never zeroed, a lookup counts only when the row it
//                                 names holds that root
//   2. obj_count_kernel           one lane per pixel, a wave on 64 consecutive pixels of one sample: label, lookup, one coalesced byte of
//                                 the annotation; the pixels of row r under object o go by one LDS atomic per horizontal run of the wave
//                                 (wave_runs.h, keyed on r O + o - 1) into the workgroup's k x O partials, the objects' own pixels by one per
//                                 run (keyed on o - 1) into its O partials, the two counts by ballots; then one 64-bit integer atomic per
//                                 non-zero partial.  The partials are dynamic LDS, (k O + O) ints: 8.3 KB at k = 64, O = 32
// Two launches whatever n, k, O and the content are; integer atomics only, no workgroup waits for another: exact, identical from run
// to run and for a sample alone or inside a batch.  A label outside 1..H_i*W_i is background, a looked-up rank counts only below the
// frame's rows and an object byte only in 1..O, so nothing indexes outside its own sample or its own tables whatever labels, dets,
// counts, objects and the workspace hold; offsets / hw are validated by the host caller (native_objects.object_overlaps).
#include "common.h"
#include "host_checks.h"
#include "track_rows.h"
#include "wave_runs.h"

namespace udet {

#define OBJ_PPT 16  // pixels per thread of the count grid: 4096 pixels per workgroup amortise the flush of k O + O partials
#define OBJ_K UDET_DET_MAX_K

__global__ __launch_bounds__(256) void obj_init_kernel(int n, const long long* __restrict__ offsets, const int* __restrict__ hw,
                                                       const long long* __restrict__ dets, const long long* __restrict__ counts, int k,
                                                       int O, unsigned long long* __restrict__ row_obj,
                                                       unsigned long long* __restrict__ obj_area,
                                                       unsigned long long* __restrict__ frame_stats, int* __restrict__ lookup) {
  const size_t stride = (size_t)gridDim.x * 256, g = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t j = g; j < (size_t)n * k; j += stride) {
    const int i = (int)(j / k), r = (int)(j - (size_t)i * k);
    link_enter_roots(dets + (size_t)i * k * UDET_DET_FIELDS, link_rows(counts + 3 * i, k), (long long)hw[2 * i] * hw[2 * i + 1],
                     lookup + offsets[i], r);
  }
  for (size_t j = g; j < (size_t)n * k * O; j += stride) row_obj[j] = 0;
  for (size_t j = g; j < (size_t)n * O; j += stride) obj_area[j] = 0;
  for (size_t j = g; j < (size_t)2 * n; j += stride) frame_stats[j] = 0;
}

__global__ __launch_bounds__(256) void obj_count_kernel(const int* __restrict__ labels, const long long* __restrict__ offsets,
                                                        const int* __restrict__ hw, const long long* __restrict__ dets,
                                                        const long long* __restrict__ counts, int k,
                                                        const unsigned char* __restrict__ objects, int O, const int* __restrict__ lookup,
                                                        unsigned long long* __restrict__ row_obj,
                                                        unsigned long long* __restrict__ obj_area,
                                                        unsigned long long* __restrict__ frame_stats) {
  extern __shared__ int part[];  // [k O] pairs, then [O] areas
  __shared__ int root_s[OBJ_K], st[2];
  const int i = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int W = hw[2 * i + 1];
  const long long HW = (long long)hw[2 * i] * W, off = offsets[i];
  if ((long long)blockIdx.x * 256 >= HW) return;  // beyond this sample's pixels (the whole workgroup)
  const int rows = link_rows(counts + 3 * i, k);
  const int kO = k * O;
  int* __restrict__ area_s = part + kO;
  for (int j = t; j < k; j += 256) {
    const long long root = j < rows ? dets[((size_t)i * k + j) * UDET_DET_FIELDS] : -1;
    root_s[j] = (root >= 0 && root < HW) ? (int)root : -1;
  }
  for (int j = t; j < kO + O; j += 256) part[j] = 0;
  if (t < 2) st[t] = 0;
  __syncthreads();
  const int* __restrict__ lab = labels + off;
  const int* __restrict__ look = lookup + off;
  const unsigned char* __restrict__ ann = objects + off;
  int n_obj = 0, n_void = 0;  // of this wave
  for (long long base = (long long)blockIdx.x * 256; base < HW; base += (long long)gridDim.x * 256) {  // block-uniform bounds
    const long long p = base + t;
    const bool valid = p < HW;
    const int L = valid ? lab[p] : 0;
    const int b = valid ? (int)ann[p] : 0;
    const int o = (b >= 1 && b <= O) ? b - 1 : -1;
    int r = -1;
    if (o >= 0 && L >= 1 && L <= HW) {
      const int c = look[L - 1];  // never zeroed: only a rank whose row holds this root counts
      if ((unsigned)c < (unsigned)rows && root_s[c] == L - 1) r = c;
    }
    const int x = valid ? (int)(p % W) : 0;
    const int pair = r >= 0 ? r * O + o : -1;
    const int len_pair = det_run_length(pair, x, lane);
    if (len_pair) atomicAdd(part + pair, len_pair);  // a workgroup sees fewer than 2^31 pixels
    const int len_obj = det_run_length(o, x, lane);
    if (len_obj) atomicAdd(area_s + o, len_obj);
    n_obj += __popcll(__ballot(o >= 0));
    n_void += __popcll(__ballot(b > O));
  }
  if (lane == 0) {
    if (n_obj) atomicAdd(st + 0, n_obj);
    if (n_void) atomicAdd(st + 1, n_void);
  }
  __syncthreads();
  for (int j = t; j < kO; j += 256)
    if (part[j]) atomicAdd(row_obj + (size_t)i * kO + j, (unsigned long long)part[j]);
  for (int j = t; j < O; j += 256)
    if (area_s[j]) atomicAdd(obj_area + (size_t)i * O + j, (unsigned long long)area_s[j]);
  if (t < 2 && st[t]) atomicAdd(frame_stats + (size_t)2 * i + t, (unsigned long long)st[t]);
}

}  // namespace udet

using namespace udet;

extern "C" {

size_t udet_track_object_overlaps_workspace_bytes(size_t total_pixels, int n, int k) {
  if (n < 1 || n > 65535 || total_pixels < 1 || k < 1 || k > UDET_DET_MAX_K) return 0;
  return total_pixels * sizeof(int);  // the root-to-rank lookup; no per-sample term
}

int udet_track_object_overlaps_ragged(const int* labels, int n, const long long* offsets, const int* hw, int max_h, int max_w,
                                      size_t total_pixels, const long long* dets, const long long* counts, int k,
                                      const unsigned char* objects, int num_objects, long long* row_obj, long long* obj_area,
                                      long long* frame_stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch("track_object_overlaps_ragged", n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (!labels || !offsets || !hw || !dets || !counts || !objects || !row_obj || !obj_area || !frame_stats) {
    set_error("track_object_overlaps_ragged: bad argument (non-null labels, offsets, hw, dets, counts, objects, row_obj, obj_area and "
              "frame_stats)");
    return UDET_ERR_ARG;
  }
  if (k < 1 || k > UDET_DET_MAX_K) {
    set_error("track_object_overlaps_ragged: k = %d in 1..UDET_DET_MAX_K = %d is required", k, UDET_DET_MAX_K);
    return UDET_ERR_ARG;
  }
  if (num_objects < 1 || num_objects > UDET_MAX_OBJECTS) {
    set_error("track_object_overlaps_ragged: num_objects = %d in 1..UDET_MAX_OBJECTS = %d is required", num_objects, UDET_MAX_OBJECTS);
    return UDET_ERR_ARG;
  }
  if (bad_workspace("track_object_overlaps_ragged", workspace, workspace_bytes,
                    udet_track_object_overlaps_workspace_bytes(total_pixels, n, k), 4))
    return UDET_ERR_ARG;
  const uintptr_t a8 = reinterpret_cast<uintptr_t>(dets) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(row_obj) |
                       reinterpret_cast<uintptr_t>(obj_area) | reinterpret_cast<uintptr_t>(frame_stats);
  if ((reinterpret_cast<uintptr_t>(labels) & 3) || (a8 & 7)) {
    set_error("track_object_overlaps_ragged: labels must be 4-byte aligned, dets, counts, row_obj, obj_area and frame_stats 8-byte aligned");
    return UDET_ERR_ARG;
  }
  const long nb = ((long)max_h * max_w + 256 * OBJ_PPT - 1) / (256 * OBJ_PPT);
  const size_t nz = ((size_t)n * k * num_objects + 255) / 256;
  const size_t lds = ((size_t)k * num_objects + num_objects) * sizeof(int);
  int* lookup = (int*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(obj_init_kernel, dim3((unsigned)(nz > 65536 ? 65536 : nz)), dim3(256), 0, s, n, offsets, hw, dets, counts, k,
                     num_objects, (unsigned long long*)row_obj, (unsigned long long*)obj_area, (unsigned long long*)frame_stats, lookup);
  hipLaunchKernelGGL(obj_count_kernel, dim3((unsigned)nb, n), dim3(256), lds, s, labels, offsets, hw, dets, counts, k, objects, num_objects,
                     lookup, (unsigned long long*)row_obj, (unsigned long long*)obj_area, (unsigned long long*)frame_stats);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // extern "C"
