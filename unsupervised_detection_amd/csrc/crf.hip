// Dense CRF of a ragged batch at each frame's own size: the mean field of post_processing/crf_refine.py:110-130 with the
// definition of udet_post_dense_crf (postproc.hip) and oracle/oracle_post.py dense_crf -- one bilateral Potts term, the Gaussian kernel
//   k_ij = exp(-|dp|^2 / 2 sxy^2 - |dI|^2 / 2 srgb^2),  |dy|, |dx| <= R,  j != i,  j inside the frame
// evaluated exactly, symmetric normalisation n_i = 1 / sqrt(sum_j k_ij + 1e-20) -- on the packed layout of restore.hip / components.hip
// (sample i = H_i x W_i elements at offsets[i]).  One kernel, crf_ragged_kernel, is the whole hot path; a call is iters + 2 launches of it
// whatever the batch size:
//   mode 0   K 1                -> norm = 1 / sqrt(. + 1e-20)
//   mode 1   K norm             -> kn;  Q = softmax(-unary);  field[0] = norm * Q1
//   mode 2   K field[cur]       -> Q = softmax(-unary + compat * norm * (kn - ., .));  field[1 - cur] = norm * Q1     (iters times)
// and the last launch also writes q1 / labels.  (Q0 = 1 - Q1, so K (norm Q0) = kn - K (norm Q1): one field is filtered per iteration.)
//
// The filter.  A workgroup of four waves owns a tile of 64 columns x 4 P rows of one sample; lane l of wave w holds the P targets
// (Y0 + w P + p, X0 + l), their colours and sums in registers.  The window is walked in blocks staged in LDS as float4 (r, g, b, field):
// CRF_S source rows (a strip, aligned to multiples of CRF_S in the frame) x 64 + CRF_DC - 1 columns (the columns the tile's 64 lanes
// reach with CRF_DC consecutive dx) -- 16 KiB whatever the radius.  Elements outside the frame are staged as zeros, so the inner loop
// has no bounds check and the frame border no code path of its own.  For one dx every lane reads the strip's CRF_S sources of its column
// x + dx (ds_read_b128, consecutive lanes 16 bytes apart: conflict-free) and each serves its P targets:
//   3 subtractions, 1 multiplication, 2 FMAs (|dI|^2, exact: integers below 2^24), 1 FMA (exponent), v_exp_f32, 1 FMA (sum)
// with exp(a + b + c) split as exp2(c2 |dI|^2 + c1 dy^2) * exp2(c1 dx^2): the row term is one of CRF_S + P - 1 wave-uniform values per
// strip (-1e30 for a row outside the target's window: the tap becomes exp2(-1e30) = 0 without a select), the column factor multiplies the
// strip's partial sum once per dx.  The tap j = i is excluded by construction: the dx = 0 pass uses row terms whose dy = 0 entry is
// -1e30 (subtracting the field's own value afterwards would cancel against a sum thousands of times larger).  With P >= 2 the targets
// are held in pairs and the same operations are written on two-float vectors (crf_column2: packed float32 instructions, two IEEE
// operations each, so the sums are those of the scalar form bit for bit; only the dx = 0 column runs the scalar form).  A wave skips the strips
// none of whose rows its targets see; blocks that lie outside the frame are skipped by the whole workgroup.
// The order in which a target's taps are summed -- strips by frame row, dx ascending, rows ascending inside a strip -- depends on
// neither P, the tile nor the batch, every multiply-add is an explicit fmaf (the file is compiled with -ffp-contract=off), there are no
// atomics and no workgroup reads what another writes in the same launch: results are bit-identical from run to run and between a
// sample run alone and inside a batch.  Every index comes from offsets / hw, which the caller validates on the host
// (native_results.check_crf_tables); staged reads are bounded by the frame, stores by x < W, y < H.
#include <math.h>

#include "common.h"
#include "host_checks.h"

namespace udet {

#define CRF_TW 64                      // tile columns: one lane each
#define CRF_S 8                        // source rows per staged strip
#define CRF_DC 64                      // consecutive dx per staged block
#define CRF_CW (CRF_TW + CRF_DC)       // staged columns (CRF_TW + CRF_DC - 1 are read), a power of two
#define CRF_OUT (-1e30f)               // exponent of a tap outside the window

struct CrfArgs {
  const unsigned char* image;  // packed rgb, 3 bytes per element
  const long long* offsets;
  const int* hw;
  const float* field_in;       // null: 1 inside the frame (mode 0)
  const float* unary;          // [2][total]
  float* norm;
  float* kn;
  float* field_out;
  float* q1;                   // written when `last`; either may be null
  unsigned char* labels;
  size_t total;
  int R, mode, last;
  float c1, c2, compat;        // -log2(e) / 2 sxy^2, -log2(e) / 2 srgb^2
};

// one dx of a staged strip: in[p] = sum_s exp2(c2 |dI|^2 + rt[s - p + P - 1]) * field_s, acc[p] += exp2(c1 dx^2) * in[p]
template <int P>
__device__ __forceinline__ void crf_column(const float4* __restrict__ col, const float (&rt)[CRF_S + P - 1], const float (&cr)[P],
                                           const float (&cg)[P], const float (&cb)[P], float c2, float wx, float (&acc)[P]) {
  float in[P];
#pragma unroll
  for (int p = 0; p < P; ++p) in[p] = 0.f;
#pragma unroll
  for (int s = 0; s < CRF_S; ++s) {
    const float4 f = col[s * CRF_CW];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float dr = cr[p] - f.x, dg = cg[p] - f.y, db = cb[p] - f.z;
      const float d2 = fmaf(db, db, fmaf(dg, dg, dr * dr));
      const float k = __builtin_amdgcn_exp2f(fmaf(d2, c2, rt[s - p + P - 1]));
      in[p] = fmaf(k, f.w, in[p]);
    }
  }
#pragma unroll
  for (int p = 0; p < P; ++p) acc[p] = fmaf(wx, in[p], acc[p]);
}

// The same for two targets at once (rows p0 and p0 + 1 of the lane's column) on packed float32 instructions (v_pk_add_f32 / v_pk_mul_f32 /
// v_pk_fma_f32: two IEEE operations each, so every sum is the one crf_column forms).  rt2[j] = (rt[j], rt[j - 1]), the row terms of the pair.
typedef float f2 __attribute__((ext_vector_type(2)));
template <int P>
__device__ __forceinline__ void crf_column2(const float4* __restrict__ col, const f2 (&rt2)[CRF_S + P - 1], const f2 (&cr)[P / 2],
                                            const f2 (&cg)[P / 2], const f2 (&cb)[P / 2], float c2, float wx, f2 (&acc)[P / 2]) {
  f2 in[P / 2];
#pragma unroll
  for (int q = 0; q < P / 2; ++q) in[q] = (f2)(0.f);
#pragma unroll
  for (int s = 0; s < CRF_S; ++s) {
    const float4 f = col[s * CRF_CW];
#pragma unroll
    for (int q = 0; q < P / 2; ++q) {
      const f2 dr = cr[q] - (f2)(f.x), dg = cg[q] - (f2)(f.y), db = cb[q] - (f2)(f.z);
      const f2 d2 = __builtin_elementwise_fma(db, db, __builtin_elementwise_fma(dg, dg, dr * dr));
      const f2 e = __builtin_elementwise_fma(d2, (f2)(c2), rt2[s - 2 * q + P - 1]);
      f2 k;
      k.x = __builtin_amdgcn_exp2f(e.x);
      k.y = __builtin_amdgcn_exp2f(e.y);
      in[q] = __builtin_elementwise_fma(k, (f2)(f.w), in[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < P / 2; ++q) acc[q] = __builtin_elementwise_fma((f2)(wx), in[q], acc[q]);
}

template <int P>
__global__ __launch_bounds__(256) void crf_ragged_kernel(const CrfArgs a) {
  __shared__ float4 tile[CRF_S * CRF_CW];
  constexpr int TH = 4 * P;
  const int i = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int H = a.hw[2 * i], W = a.hw[2 * i + 1];
  const int tiles_x = (W + CRF_TW - 1) / CRF_TW, tiles_y = (H + TH - 1) / TH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // block-uniform: the grid is sized for the largest frame of the batch
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = tx * CRF_TW, Y0 = ty * TH, x = X0 + lane, yw = Y0 + wv * P;
  const size_t o = (size_t)a.offsets[i];
  const unsigned char* __restrict__ img = a.image + 3 * o;
  const float* __restrict__ fin = a.field_in ? a.field_in + o : nullptr;
  const int R = a.R;
  const float c1 = a.c1, c2 = a.c2;

  float cr[P], cg[P], cb[P], acc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int y = yw + p;
    const size_t k = (x < W && y < H) ? (size_t)y * W + x : 0;  // a lane outside the frame computes on pixel 0 and stores nothing
    cr[p] = (float)img[3 * k];
    cg[p] = (float)img[3 * k + 1];
    cb[p] = (float)img[3 * k + 2];
    acc[p] = 0.f;
  }

  constexpr int P2 = P >= 2 ? P / 2 : 1;
  f2 cr2[P2], cg2[P2], cb2[P2], acc2[P2];  // P >= 2: the same in pairs, for the packed instructions of crf_column2
#pragma unroll
  for (int q = 0; q < P2; ++q) {
    cr2[q] = (f2){cr[(2 * q) % P], cr[(2 * q + 1) % P]};
    cg2[q] = (f2){cg[(2 * q) % P], cg[(2 * q + 1) % P]};
    cb2[q] = (f2){cb[(2 * q) % P], cb[(2 * q + 1) % P]};
    acc2[q] = (f2)(0.f);
  }

  const int r0 = Y0 - R > 0 ? Y0 - R : 0, r1 = Y0 + TH - 1 + R < H - 1 ? Y0 + TH - 1 + R : H - 1;
  for (int sy = r0 / CRF_S * CRF_S; sy <= r1; sy += CRF_S) {
    // wave-uniform row terms of the strip: source row sy + s and target row yw + p are dy = (sy - yw) + (s - p) apart
    float rtn[CRF_S + P - 1];
#pragma unroll
    for (int j = 0; j < CRF_S + P - 1; ++j) {
      const int dy = sy - yw + j - (P - 1);
      rtn[j] = (dy >= -R && dy <= R) ? c1 * ((float)dy * (float)dy) : CRF_OUT;
    }
    f2 rt2[CRF_S + P - 1];  // P >= 2: the row terms of a pair of targets
#pragma unroll
    for (int j = 1; j < CRF_S + P - 1; ++j) rt2[j] = (f2){rtn[j], rtn[j - 1]};
    const bool wave_sees = sy + CRF_S - 1 >= yw - R && sy <= yw + P - 1 + R;
    for (int d0 = -R; d0 <= R; d0 += CRF_DC) {
      const int jn = R - d0 + 1 < CRF_DC ? R - d0 + 1 : CRF_DC;
      const int col0 = X0 + d0;  // staged columns col0 .. col0 + CRF_CW - 1; read: col0 .. col0 + CRF_TW + jn - 2
      if (col0 + CRF_TW + jn - 2 < 0 || col0 >= W) continue;  // block-uniform
      __syncthreads();
      for (int e = t; e < CRF_S * CRF_CW; e += 256) {
        const int yy = sy + e / CRF_CW, xx = col0 + (e & (CRF_CW - 1));
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (yy < H && xx >= 0 && xx < W) {  // (yy >= 0: strips start inside the frame)
          const size_t k = (size_t)yy * W + xx;
          v = make_float4((float)img[3 * k], (float)img[3 * k + 1], (float)img[3 * k + 2], fin ? fin[k] : 1.f);
        }
        tile[e] = v;
      }
      __syncthreads();
      if (!wave_sees) continue;  // wave-uniform; the barriers above are passed by every wave
      for (int j = 0; j < jn; ++j) {
        const float fdx = (float)(d0 + j);
        const float wx = __builtin_amdgcn_exp2f(c1 * (fdx * fdx));
        if (d0 + j == 0) {  // no tap j = i: the row terms of this one column have -1e30 at dy = 0
          float rts[CRF_S + P - 1];
#pragma unroll
          for (int m = 0; m < CRF_S + P - 1; ++m) rts[m] = sy - yw + m - (P - 1) == 0 ? CRF_OUT : rtn[m];
          if constexpr (P >= 2) {
            float as[P];
#pragma unroll
            for (int q = 0; q < P / 2; ++q) { as[2 * q] = acc2[q].x; as[2 * q + 1] = acc2[q].y; }
            crf_column<P>(tile + lane + j, rts, cr, cg, cb, c2, wx, as);
#pragma unroll
            for (int q = 0; q < P / 2; ++q) acc2[q] = (f2){as[2 * q], as[2 * q + 1]};
          } else {
            crf_column<P>(tile + lane + j, rts, cr, cg, cb, c2, wx, acc);
          }
        } else if constexpr (P >= 2) {
          crf_column2<P>(tile + lane + j, rt2, cr2, cg2, cb2, c2, wx, acc2);
        } else {
          crf_column<P>(tile + lane + j, rtn, cr, cg, cb, c2, wx, acc);
        }
      }
    }
  }

  if constexpr (P >= 2) {
#pragma unroll
    for (int q = 0; q < P / 2; ++q) { acc[2 * q] = acc2[q].x; acc[2 * q + 1] = acc2[q].y; }
  }
  if (x >= W) return;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int y = yw + p;
    if (y >= H) break;
    const size_t k = o + (size_t)y * W + x;
    if (a.mode == 0) {
      a.norm[k] = 1.f / sqrtf(acc[p] + 1e-20f);
      continue;
    }
    const float nrm = a.norm[k];
    float e0 = -a.unary[k], e1 = -a.unary[a.total + k];
    if (a.mode == 1) {
      a.kn[k] = acc[p];
    } else {
      const float m1 = nrm * acc[p], m0 = nrm * (a.kn[k] - acc[p]);
      e0 += a.compat * m0;
      e1 += a.compat * m1;
    }
    const float mx = fmaxf(e0, e1);
    const float p0 = expf(e0 - mx), p1 = expf(e1 - mx), s = p0 + p1;
    const float q0 = p0 / s, q1 = p1 / s;
    a.field_out[k] = nrm * q1;
    if (a.last) {
      if (a.q1) a.q1[k] = q1;
      if (a.labels) a.labels[k] = q1 > q0 ? 1 : 0;  // np.argmax: label 1 only where strictly larger
    }
  }
}

// unary[l][o_i + k] = table[i][l][data[o_i + k]]: the two energies of crf_refine.py:113-121 as a function of the restored byte
__global__ __launch_bounds__(256) void crf_unary_lookup_kernel(const unsigned char* __restrict__ data, const float* __restrict__ table,
                                                               const long long* __restrict__ offsets, const int* __restrict__ hw,
                                                               size_t total, float* __restrict__ unary) {
  const int i = blockIdx.y;
  const long long HW = (long long)hw[2 * i] * hw[2 * i + 1];
  const size_t o = (size_t)offsets[i];
  const float* __restrict__ tab = table + (size_t)i * 512;
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < HW; k += (long long)gridDim.x * 256) {
    const int b = data[o + k];
    unary[o + k] = tab[b];
    unary[total + o + k] = tab[256 + b];
  }
}

template <int P>
static void crf_launch(const CrfArgs& a, int n, int max_h, int max_w, hipStream_t s) {
  const unsigned tiles = (unsigned)(((max_w + CRF_TW - 1) / CRF_TW) * ((max_h + 4 * P - 1) / (4 * P)));
  hipLaunchKernelGGL(crf_ragged_kernel<P>, dim3(tiles, n), dim3(256), 0, s, a);
}

}  // namespace udet

using namespace udet;

extern "C" {

size_t udet_dense_crf_workspace_bytes(size_t total_pixels, int n) {
  return (n < 1 || total_pixels < 1) ? 0 : 4 * total_pixels * sizeof(float);  // norm, K norm, two fields
}

// rows per thread (the sums do not depend on it): the form with the smallest estimated time, rounds x cost of a workgroup, ties to more
// rows.  rounds = workgroups / 256 CUs, rounded up (a partly filled last round costs a whole one) and at least 2 (below two waves per SIMD
// a wave issues at half rate, so a smaller grid is no faster); cost = 52 / 66 / 120: the measured cycles per pair and row of the scalar
// 1-row form and of the packed 2- and 4-row forms (profiles/NOTES.md has the three measurements this is fitted to).
int udet_dense_crf_rows_per_thread(int n, int max_h, int max_w) {
  if (n < 1 || max_h < 1 || max_w < 1) return 0;
  const long long cols = (max_w + CRF_TW - 1) / CRF_TW;
  int best = 1;
  long long best_t = 0;
  for (int P = 1; P <= 4; P *= 2) {
    const long long wg = cols * ((max_h + 4 * P - 1) / (4 * P)) * n;
    const long long rounds = (wg + 255) / 256;
    const long long t = (rounds > 2 ? rounds : 2) * (P == 1 ? 52 : (P == 2 ? 66 : 120));
    if (P == 1 || t <= best_t) { best = P; best_t = t; }
  }
  return best;
}

int udet_dense_crf_ragged(const float* unary, const unsigned char* image_rgb, int n, const long long* offsets, const int* hw, int max_h,
                          int max_w, size_t total_pixels, float sxy, float srgb, float compat, int iters, int radius, float* q1,
                          unsigned char* labels, void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_batch("dense_crf_ragged", n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (!unary || !image_rgb || !offsets || !hw) {
    set_error("dense_crf_ragged: bad argument (non-null unary, image_rgb, offsets and hw)");
    return UDET_ERR_ARG;
  }
  if (iters < 0 || radius < 1 || !(sxy > 0.f) || !(srgb > 0.f) || isinf(sxy) || isinf(srgb)) {
    set_error("dense_crf_ragged: iters %d >= 0, radius %d >= 1, finite sxy %g > 0 and srgb %g > 0 are required", iters, radius, sxy, srgb);
    return UDET_ERR_ARG;
  }
  if (!q1 && !labels) {
    set_error("dense_crf_ragged: at least one of q1 and labels must be given");
    return UDET_ERR_ARG;
  }
  if (reinterpret_cast<uintptr_t>(q1) & 3) {
    set_error("dense_crf_ragged: q1 must be 4-byte aligned");
    return UDET_ERR_ARG;
  }
  if (bad_workspace("dense_crf_ragged", workspace, workspace_bytes, udet_dense_crf_workspace_bytes(total_pixels, n), 16)) return UDET_ERR_ARG;
  if (max_h > (1 << 29) || max_w > (1 << 29)) {  // tile and window coordinates are 32-bit
    set_error("dense_crf_ragged: a frame side above 2^29 is not supported");
    return UDET_ERR_SHAPE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  float* field[2] = {ws + 2 * total_pixels, ws + 3 * total_pixels};
  CrfArgs a;
  a.image = image_rgb; a.offsets = offsets; a.hw = hw; a.unary = unary;
  a.norm = ws; a.kn = ws + total_pixels;
  a.q1 = q1; a.labels = labels; a.total = total_pixels;
  const int side = max_h > max_w ? max_h : max_w;
  a.R = radius < side ? radius : side;  // a window wider than the largest frame sees nothing more
  a.c1 = (float)(-0.5 * 1.4426950408889634 / ((double)sxy * sxy));
  a.c2 = (float)(-0.5 * 1.4426950408889634 / ((double)srgb * srgb));
  a.compat = compat;
  const int P = udet_dense_crf_rows_per_thread(n, max_h, max_w);
  for (int l = 0; l < iters + 2; ++l) {
    a.mode = l < 2 ? l : 2;
    a.last = l == iters + 1;
    a.field_in = l == 0 ? nullptr : (l == 1 ? a.norm : field[l & 1]);
    a.field_out = field[(l + 1) & 1];
    if (P == 4) crf_launch<4>(a, n, max_h, max_w, s);
    else if (P == 2) crf_launch<2>(a, n, max_h, max_w, s);
    else crf_launch<1>(a, n, max_h, max_w, s);
  }
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

int udet_crf_unary_lookup(const unsigned char* data, const float* table, int n, const long long* offsets, const int* hw, int max_h,
                          int max_w, size_t total_pixels, float* unary, void* stream) {
  if (bad_batch("crf_unary_lookup", n, max_h, max_w, total_pixels)) return UDET_ERR_ARG;
  if (!data || !table || !offsets || !hw || !unary || (reinterpret_cast<uintptr_t>(unary) & 3) || (reinterpret_cast<uintptr_t>(table) & 3)) {
    set_error("crf_unary_lookup: bad argument (non-null data, offsets and hw, non-null 4-byte aligned table and unary)");
    return UDET_ERR_ARG;
  }
  const long nb = ((long)max_h * max_w + 2047) / 2048;
  hipLaunchKernelGGL(crf_unary_lookup_kernel, dim3((unsigned)nb, n), dim3(256), 0, (hipStream_t)stream, data, table, offsets, hw,
                     total_pixels, unary);
  UDET_HIP(hipGetLastError());
  return UDET_OK;
}

}  // extern "C"
