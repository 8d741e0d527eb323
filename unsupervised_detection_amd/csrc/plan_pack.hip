// Plan execution, packing: the workspace's one-off initialisation (device tables of the weight re-layout jobs and of the segmented
// launches) and the calls that re-lay the networks' weights out for the kernels.
#include <string.h>

#include "conv_host.h"
#include "plan_run.h"

namespace udet {

// ------------------------------------------------------- init / packing ----
// up-conv algebra of the recover decoder: four forward and four backward-data weight sets (pack modes 9 / 10), set
// r = (last row) + 2 (last column) -> job variant (row, column) in {interior, last}
void upb_pack_jobs(const Layer& L, const PackJob& base, std::vector<PackJob>& jobs) {
  PackJob j = base;
  for (int r = 0; r < 4; ++r) {
    j.T = 36; j.gamma_off = -1;
    j.dst_off = (long)(L.wupb_off + (size_t)r * 36 * L.Kc * L.ldw); j.R = L.cin; j.C = L.cout; j.Kc = L.Kc; j.ldw = L.ldw; j.k_split = L.k_split; j.k_gap = L.k_gap;
    j.mode = 9; j.beta_off = (long)((r & 1) * 3 + (r >> 1)); j.total = (long)L.Kc * L.ldw;  // (one work item per (k, n))
    jobs.push_back(j);
    if (L.upb_bwd) {  // (a level that keeps the up-sampled form for backward-data never reads these)
      j.dst_off = (long)(L.wupbT_off + (size_t)r * 36 * L.KcT * L.ldwT); j.Kc = L.KcT; j.ldw = L.ldwT; j.k_split = L.KcT; j.k_gap = 0;
      j.mode = 10; j.total = (long)L.KcT * L.ldwT;
      jobs.push_back(j);
    }
  }
}

int plan_init_workspace(Plan* P, float* ws, hipStream_t s) {
  UDET_HIP(hipMemsetAsync(ws, 0, P->arena_floats * sizeof(float), s));
  for (int net = 1; net <= 2; ++net) {
    const NetParams& np = net_params(net);
    std::vector<long> tab(2 * np.p.size());
    for (size_t i = 0; i < np.p.size(); ++i) {
      tab[i] = (long)np.p[i].offset;
      tab[np.p.size() + i] = (long)np.p[i].count;
    }
    UDET_HIP(hipMemcpyAsync(ws + P->seg_off[net], tab.data(), tab.size() * sizeof(long), hipMemcpyHostToDevice, s));
    UDET_HIP(hipStreamSynchronize(s));  // `tab` is a host temporary
  }
  // weight re-layout job tables of the trainable networks (one launch per network and step)
  for (int net = 1; net <= 2; ++net) {
    const NetParams& np = net_params(net);
    const std::vector<Layer>& layers = net == NET_GEN ? P->gen : P->rec;
    std::vector<PackJob> jobs;
    for (const auto& L : layers) {
      const int T = L.kh * L.kw;
      const long goff = L.g_idx >= 0 ? (long)np.p[L.g_idx].offset : -1, beoff = L.be_idx >= 0 ? (long)np.p[L.be_idx].offset : -1;
      PackJob j;
      memset(&j, 0, sizeof(j));
      j.src_off = (long)np.p[L.w_idx].offset; j.gamma_off = goff; j.beta_off = beoff;
      j.T = T;
      // forward operand (conv2d_transpose layers store [t][cout][cin] and never occur in the trainable nets)
      j.dst_off = (long)L.wp_off; j.R = L.cin; j.C = L.cout; j.Kc = L.Kc; j.ldw = L.ldw; j.k_split = L.k_split; j.k_gap = L.k_gap;
      j.mode = 0; j.total = (long)T * L.Kc * L.ldw;
      jobs.push_back(j);
      // transposed operand of the backward-data pass
      j.dst_off = (long)L.wpT_off; j.Kc = L.KcT; j.ldw = L.ldwT; j.k_split = L.KcT; j.k_gap = 0;
      j.mode = 1; j.total = (long)T * L.KcT * L.ldwT;
      jobs.push_back(j);
      if (L.col2im) {  // taps folded into the N axis (GEMM + gather heads)
        j.dst_off = (long)L.wz_off; j.R = L.cin; j.C = L.cout; j.Kc = L.Kc; j.ldw = L.ldz; j.k_split = L.k_split; j.k_gap = L.k_gap;
        j.mode = 3; j.total = (long)L.Kc * L.ldz;
        jobs.push_back(j);
      }
      if (L.up) {  // NN x2 + 3x3 as four 2x2 convolutions on the low-resolution grid (run_fwd / run_dgrad)
        j.T = 16;
        j.dst_off = (long)L.wu_off; j.R = L.cin; j.C = L.cout; j.Kc = L.Kc; j.ldw = L.ldw; j.k_split = L.Kc; j.k_gap = 0;
        j.mode = 5; j.total = (long)16 * L.Kc * L.ldw;
        jobs.push_back(j);
        j.dst_off = (long)L.wuT_off; j.Kc = L.KcT; j.ldw = L.ldwT; j.k_split = L.KcT; j.k_gap = 0;
        j.mode = 6; j.total = (long)16 * L.KcT * L.ldwT;
        jobs.push_back(j);
        j.T = T;
      }
      if (L.upb) upb_pack_jobs(L, j, jobs);
      if (L.wino_off) {  // Winograd operand of the forward pass: K = input channels with the slab's gap map, N = output channels
        j.dst_off = (long)L.wino_off; j.R = L.cin; j.C = L.cout; j.Kc = L.Kc; j.ldw = L.wino_np; j.k_split = L.k_split; j.k_gap = L.k_gap;
        j.mode = 7; j.total = (long)(L.Kc / 8) * 2 * L.wino_np;  // work items (wino_pack.h)
        jobs.push_back(j);
      }
      if (L.winoT_off) {  // ... of the backward-data pass: K = output channels, N = input channels, taps mirrored
        j.dst_off = (long)L.winoT_off; j.R = L.cin; j.C = L.cout; j.Kc = L.KcT; j.ldw = L.winoT_np; j.k_split = L.KcT; j.k_gap = 0;
        j.mode = 8; j.total = (long)(L.KcT / 8) * 2 * L.winoT_np;
        jobs.push_back(j);
      }
      // bias (BN-folded for the generator)
      j.src_off = (long)np.p[L.b_idx].offset; j.dst_off = (long)L.bias_f_off; j.mode = 2; j.total = L.cout;
      jobs.push_back(j);
    }
    if (jobs.size() > UDET_PACKJOB_CAP(layers.size())) {  // (the arena reserves exactly that many entries: plan_build)
      set_error("plan_init: %zu weight re-layout jobs for %zu layers exceed the table's %zu entries", jobs.size(), layers.size(),
                (size_t)UDET_PACKJOB_CAP(layers.size()));
      return UDET_ERR_ARG;
    }
    P->njobs[net] = (int)jobs.size();
    UDET_HIP(hipMemcpyAsync(ws + P->jobs_off[net], jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice, s));
    UDET_HIP(hipStreamSynchronize(s));  // `jobs` is a host temporary
  }
  for (const auto& L : P->rec)  // tap tables of the segmented launches (recover decoder's up-conv algebra)
    if (L.upb)
      for (const Layer::SegLaunch* g : {&L.upb_f, &L.upb_b})
        if (g == &L.upb_f || L.upb_bwd)
          UDET_HIP(hipMemcpyAsync(ws + g->tab_off, g->taps.data(), g->taps.size() * sizeof(ConvTap), hipMemcpyHostToDevice, s));
  UDET_HIP(hipStreamSynchronize(s));
  P->pwc_packed = false;
  return UDET_OK;
}

static int pack_layer(const Layer& L, const float* w_flat, float* ws, const float* scale, bool trainable, hipStream_t s) {
  const NetParams& np = net_params(L.net);
  const float* w = w_flat + np.p[L.w_idx].offset;
  const int T = L.kh * L.kw;
  if (L.transposed)  // weights are [t][cout][cin]
    UDET_TRY(launch_pack_weights(w, ws + L.wp_off, T, L.cout, L.cin, L.Kc, L.ldw, L.k_split, L.k_gap, 1, nullptr, s));
  else
    UDET_TRY(launch_pack_weights(w, ws + L.wp_off, T, L.cin, L.cout, L.Kc, L.ldw, L.k_split, L.k_gap, 0, scale, s));
  if (trainable)
    UDET_TRY(launch_pack_weights(w, ws + L.wpT_off, T, L.cin, L.cout, L.KcT, L.ldwT, L.KcT, 0, 1, scale, s));
  if (L.col2im)
    UDET_TRY(launch_pack_taps_into_n(w, ws + L.wz_off, T, L.cin, L.cout, L.Kc, L.ldz, L.k_split, L.k_gap, L.transposed ? 1 : 0, s));
  if (L.wino_off && !trainable)  // (the trainable nets build theirs in the per-step job table, BN folded)
    UDET_TRY(launch_wino_pack(w, ws + L.wino_off, L.cin, L.cout, L.Kc, L.wino_np, L.k_split, L.k_gap, 0, s));
  return UDET_OK;
}

int plan_pack_pwc(Plan* P, const float* w, float* ws, hipStream_t s) {
  const NetParams& np = net_params(NET_PWC);
  for (const auto& L : P->pwc) {
    UDET_TRY(pack_layer(L, w, ws, nullptr, false, s));
    UDET_TRY(launch_copy_channels(w + np.p[L.b_idx].offset, L.cout, 0, ws + L.bias_f_off, L.cout, 0, 1, L.cout, 1.f, 0.f, s));
  }
  P->pwc_packed = true;
  return UDET_OK;
}

int plan_pack_trainable(Plan* P, const float* w_gen, const float* w_rec, float* ws, hipStream_t s) {
  if (w_gen)
    UDET_TRY(launch_pack_jobs(reinterpret_cast<const PackJob*>(ws + P->jobs_off[NET_GEN]), P->njobs[NET_GEN], w_gen, ws, BN_C, s));
  if (w_rec)
    UDET_TRY(launch_pack_jobs(reinterpret_cast<const PackJob*>(ws + P->jobs_off[NET_REC]), P->njobs[NET_REC], w_rec, ws, BN_C, s));
  return UDET_OK;
}

}  // namespace udet
