// Internal: what the files that execute a plan share (plan.h stays the interface to the rest of the library) --
//   plan_lanes.hip  profiling brackets, lane placement and pinning, the event pool and the order edges between lanes,
//   plan_exec.hip   the runners: one layer's forward / backward-data / filter-gradient pass as launches on a lane,
//   plan_pack.hip   workspace initialisation, the weight re-layout tables and the pack calls,
//   plan_step.hip   the walk of the step: PWC-Net, generator, recover forward, losses, the two backward passes,
//   plan_optim.hip  the optimizer apply and the fp16 overflow reports.
#pragma once
#include "plan.h"

namespace udet {

static const float BN_C = 0.99950037468777316f;  // 1/sqrt(1+1e-3): inference-mode BN with moving stats (0,1)

// ---- plan_lanes.hip -----------------------------------------------------------------------------------------------------------
// Lane 0 is the caller's stream; lanes 1..5 are placed on the plan's candidate streams by place_lanes (lanes that share a hardware
// queue are the same stream).  While profiling (per-kernel timing) or with UDET_SERIAL=1 every lane collapses onto the caller's
// stream, which reproduces the plain program order.
struct Lane {
  hipStream_t s;
  int slot;
};
Lane lane_of(Plan* P, hipStream_t main, int i);
hipEvent_t next_event(Plan* P);
// work enqueued on `to` after this call also waits for everything enqueued on `from` so far
void order_after(Plan* P, const Lane& from, const Lane& to);

// ---- plan_exec.hip ------------------------------------------------------------------------------------------------------------
// dU emission of a backward-data launch: output channels [c0,c1) of the result (relative to dx_coff) are also written,
// multiplied by act'(activation `abuf`), into `ubuf` (same layout as the dx buffer)
struct Emit {
  int ubuf = -1, abuf = -1, c0 = 0, c1 = 0, act = ACT_NONE;
  float alpha = 0.f;
};
struct DgradJob {
  const Layer* L;
  int N, dy, dx, dx_coff, accumulate;
  Emit em;
};
// (experiment knob UDET_KNOB_NO_PAIRS, libudet_exp.so only: bit 0 forward pairs off, bit 1 backward-data pairs off)
inline bool pairs_on(const Plan* P, int dir = 0) { return !P->cfg.conv_fp16 && !((plan_knob(UDET_KNOB_NO_PAIRS) >> dir) & 1); }
int run_fwd(Plan* P, const Layer& L, int N, float* ws, const Lane& ln);
int run_fwd_pair(Plan* P, const Layer& La, int Na, const Layer& Lb, int Nb, float* ws, const Lane& ln);
// gradient w.r.t. the layer input: dX(dx buffer) (=|+=) conv_T(dU) [+ res].  dy_is_du: `dy` already holds
// dU = dY * act'(saved output) (emitted by the launch that finalised dY); otherwise act' is applied on load.
int run_dgrad(Plan* P, const Layer& L, int N, int dy, bool dy_is_du, int dx, int dx_coff, int accumulate, int res, const Emit& em, float* ws,
              const Lane& ln);
// both jobs read a materialised dU (dy_is_du) and carry no residual operand
int run_dgrad_pair(Plan* P, const DgradJob& ja, const DgradJob& jb, float* ws, const Lane& ln);
// gradient w.r.t. the low-resolution source of an upb level: dsrc (written) from dU (`du` buffer, channels [0, KcT))
int run_dgrad_upb(Plan* P, const Layer& L, int N, int du, int dxhat, int dsrc, float* ws, const Lane& ln);
int run_wgrad(Plan* P, const Layer& L, int N, int dy, bool dy_is_du, const float* w_flat, float* g_flat, float* ws, const Lane& ln);
// The up-conv algebra's two passes on operands instead of plan buffers: run_fwd_upb / run_dgrad_upb fill these from the plan, the
// single-layer entry of libudet_debug (udet_debug_upconv_lowres_*) from its arguments.
struct UpbLane {  // what fill_common gives a launch: split-K slabs, the zero block, the ticket counters, the fp16 switch
  float* partial;
  size_t partial_cap;
  const float* zero16;
  int* tickets;
  int f16;
};
struct UpbFwd {
  int N, h, w;                       // low-resolution source grid
  const float* src;                  // [N, h, w, ld]
  float* xhat;                       // ringed source [N, h + 2, w + 2, ld] (written)
  int ld;
  const float* wsets;                // four weight sets [4][36][Kc][ldw] (pack mode 9)
  int Kc, ldw;
  const float* bias;
  float* y;                          // [N, 2h, 2w, ldy], channels [y_coff, y_coff + cout)
  int ldy, y_coff, cout, act;
  float alpha;
  const Layer::SegLaunch* tab;       // build_upb_launches' forward table and its device copy
  const ConvTap* tab_dev;
  bool split;                        // interior as a four-class launch + the twelve border segments (Layer::upb_split)
  UpbLane lane;
};
struct UpbBwd {
  int N, h, w;
  const float* du;                   // [N, 2h, 2w, lddu], channels [du_coff, du_coff + KcT)
  int lddu, du_coff;
  const float* wsetsT;               // [4][36][KcT][ldwT] (pack mode 10)
  int KcT, ldwT, cout;
  float* dxhat;                      // ringed gradient [N, h + 2, w + 2, ld], channels [0, cin) (written)
  float* dsrc;                       // [N, h, w, ld]: the ring's adjoint of dxhat (written)
  int ld, cin;
  const Layer::SegLaunch* tab;       // the backward-data table and its device copy
  const ConvTap* tab_dev;
  float f16_xscale;                  // fp16 mode: scale of the gradient operand
  UpbLane lane;
};
int upb_forward(const UpbFwd& a, hipStream_t s);
int upb_dgrad(const UpbBwd& a, hipStream_t s);

}  // namespace udet
