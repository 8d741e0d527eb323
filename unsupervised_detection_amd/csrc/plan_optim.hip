// Plan execution, optimizer: the clipped Adam apply of one network and, in fp16 mode, the bookkeeping of updates dropped because
// their gradients overflowed (Plan::ovf_host).
#include <math.h>

#include "elementwise.h"
#include "plan_run.h"

namespace udet {

// ------------------------------------------------------------ optimizer ----
static int overflow_consume(Plan* P, int net, bool wait);
int plan_apply(Plan* P, int net, float* w, float* g, float* m, float* v, float* ws, hipStream_t s) {
  if (net != NET_GEN && net != NET_REC) {
    set_error("apply: net must be 1 (generator) or 2 (recover)");
    return UDET_ERR_ARG;
  }
  const Config& c = P->cfg;
  const NetParams& np = net_params(net);
  float* sm = ws + P->small_off;
  const float* flag = nullptr;
  if (net == NET_GEN) {  // can_change=True (adversarial_learner.py:224-228)
    const long* tab = reinterpret_cast<const long*>(ws + P->seg_off[net]);
    UDET_TRY(launch_grad_absmean(g, tab, tab + np.p.size(), (int)np.p.size(), sm + 2048, 1e-5f, sm + UDET_SMALL_NOISE, s));
    flag = sm + UDET_SMALL_NOISE;
  }
  // fp16 mode: the report of this network's PREVIOUS apply is consumed first (normally long over: that apply is a whole step old).  A
  // dropped update gives its step count back there (overflow_consume), so the count -- the shared beta powers, udet_get_adam_step,
  // checkpoints -- equals the number of updates that really happened from the next apply on, instead of running one ahead per dropped
  // update for good.  The host cannot know at enqueue time, so the applies enqueued between a drop and its report (at most the other
  // network's, and this network's next) still use the advanced count: a transient of one step, not a persistent offset.
  if (c.conv_fp16) UDET_TRY(overflow_consume(P, net, true));
  const long t = ++P->adam_t;  // ONE optimizer object: beta powers advance on every apply (:216)
  const double lr_t = (double)c.lr * sqrt(1.0 - pow((double)c.beta2, (double)t)) / (1.0 - pow((double)c.beta1, (double)t));
  const int* skip = nullptr;
  if (c.conv_fp16) {  // overflow guard of the static fp16 gradient scale (see Plan::ovf_host)
    int* cnt = reinterpret_cast<int*>(sm + UDET_SMALL_OVF) + 2 * (net - 1);  // {this apply, running total}; view "fp16_overflow"
    UDET_TRY(launch_nonfinite_count(g, (long)np.total, cnt, s));
    skip = cnt;
  }
  UDET_TRY(launch_adam(w, g, m, v, (long)np.total, (float)lr_t, c.beta1, c.beta2, c.adam_eps, c.clip, flag, c.noise_seed,
                       (uint64_t)t, s, 0, skip));
  if (c.conv_fp16) {
    if (!P->ovf_host) UDET_HIP(hipHostMalloc(reinterpret_cast<void**>(&P->ovf_host), 4 * sizeof(int), hipHostMallocDefault));
    if (!P->ovf_ev[net]) UDET_HIP(hipEventCreateWithFlags(&P->ovf_ev[net], hipEventDisableTiming));
    // (the pinned slot and the event are re-used: the previous report was consumed above)
    UDET_HIP(hipMemcpyAsync(P->ovf_host + 2 * (net - 1), skip, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    UDET_HIP(hipEventRecord(P->ovf_ev[net], s));
    P->ovf_pending[net] = true;
  }
  return UDET_OK;
}

// looks at the pending report of `net` (wait: block until its apply has run; otherwise only if it has) and books a dropped update
static int overflow_consume(Plan* P, int net, bool wait) {
  if (!P->ovf_pending[net]) return UDET_OK;
  if (wait) UDET_HIP(hipEventSynchronize(P->ovf_ev[net]));
  else if (hipEventQuery(P->ovf_ev[net]) != hipSuccess) return UDET_OK;  // still in flight: looked at by a later call
  P->ovf_pending[net] = false;
  const int n = P->ovf_host[2 * (net - 1)];
  if (n > 0) {
    P->ovf_report_values += n; P->ovf_report_nets |= net; ++P->ovf_skipped;
    if (P->adam_t > 0) --P->adam_t;  // the dropped update did not happen: it does not count (see plan_apply)
  }
  return UDET_OK;
}

// fp16 mode: waits for the pending per-network reports and books dropped updates (adam_t gives their step back) WITHOUT raising the
// pending UDET_ERR_OVERFLOW -- that stays for the next call on the plan.  udet_get_adam_step / udet_set_adam_step go through here, so a
// count read for a checkpoint is never one ahead of the updates that really happened, and a count restored from one is not decremented
// by the report of an apply that preceded the restore.
void plan_settle_adam_step(Plan* P) {
  if (!P->cfg.conv_fp16) return;
  for (int net = 1; net <= 2; ++net) (void)overflow_consume(P, net, true);
}

int plan_check_overflow(Plan* P, bool wait) {
  if (!P->cfg.conv_fp16) return UDET_OK;
  for (int net = 1; net <= 2; ++net) UDET_TRY(overflow_consume(P, net, wait));
  if (!P->ovf_report_values) return UDET_OK;
  const int bad = P->ovf_report_values, which = P->ovf_report_nets;
  P->ovf_report_values = 0;
  P->ovf_report_nets = 0;
  set_error("fp16 mode: %d non-finite gradient value(s) in the %s gradients -- a gradient operand times 4096 overflowed fp16 (|dU| > 16); "
            "the optimizer update(s) concerned were NOT applied (weights and Adam slots unchanged)", bad,
            which == 3 ? "generator and recover" : (which == 1 ? "generator" : "recover"));
  return UDET_ERR_OVERFLOW;
}

}  // namespace udet
