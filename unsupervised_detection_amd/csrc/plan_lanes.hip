// Plan execution, lanes: which stream each of the step's independent chains runs on, the events that order them, and the
// profiling brackets around a group of launches.  See Plan::Placement (plan.h) and DESIGN.md 4.3.
#include "lanes.h"
#include "plan_run.h"

namespace udet {

// ------------------------------------------------------------ profiling ----
void prof_begin(Plan* P, int cat, double flops, double bytes, hipStream_t s, const char* name) {
  if (!P->profiling) return;
  Plan::ProfRec* r = new Plan::ProfRec();
  r->cat = cat; r->flops = flops; r->bytes = bytes; r->name = name ? name : "";
  r->sink.ev = r->kev; r->sink.n = 0; r->sink.cap = Plan::ProfRec::MAXK;
  (void)hipEventCreate(&r->a);
  (void)hipEventCreate(&r->b);
  (void)hipEventRecord(r->a, s);
  P->prof.push_back(r);
  g_launch_sink = &r->sink;  // kernels launched until prof_end carry their own start / stop events
}
void prof_end(Plan* P, hipStream_t s) {
  if (!P->profiling) return;
  g_launch_sink = nullptr;
  (void)hipEventRecord(P->prof.back()->b, s);
}

// ---------------------------------------------------------------- lanes ----
// lay the six lanes out on `n` (0..3) side streams that sit on distinct hardware queues, distinct from main's, and make that the
// placement in use for `main` (one cached placement per caller stream)
static const Plan::Placement& set_placement(Plan* P, hipStream_t main, hipStream_t const* side, int n) {
  Plan::Placement pl;
  pl.main = main;
  pl.nqueues = n + 1;
  const int q1 = n > 0 ? 1 : 0, q3 = n > 1 ? (n > 2 ? 2 : 1) : q1, q4 = n > 2 ? 3 : (n > 1 ? 2 : q1);
  // measured alternatives (ms per step; this one 10.90): lane 3 on lane 1's queue 11.20, lane 2 on its own queue and 3 with 1 11.12,
  // lane 2 with 1 11.42, lane 5 with 3 10.96 / with 1 or 0 12.2, lanes 2 and 3 swapped 10.94 (profiles/r03_hop_bench.txt)
  const int queue[Plan::NLANE] = {0, q1, 0, q3, q4, q4};
  for (int i = 0; i < Plan::NLANE; ++i) {
    pl.queue[i] = queue[i];
    pl.lane[i] = queue[i] == 0 ? main : side[queue[i] - 1];
  }
  for (size_t k = 0; k < P->placements.size(); ++k)
    if (P->placements[k].main == main) { P->placements[k] = pl; P->placed = (int)k; return P->placements[k]; }
  if (P->placements.size() >= 16) { P->placements.clear(); P->placed = -1; }  // (a caller that keeps making new streams: start over)
  P->placements.push_back(pl);
  P->placed = (int)P->placements.size() - 1;
  return P->placements[P->placed];
}
// first use from `main`: find candidate streams that run concurrently with it and with each other (one probe each, ~0.1 ms; the
// device is synchronised once) and lay the lanes out on them -- see Plan::Placement
static const Plan::Placement& place_lanes(Plan* P, hipStream_t main) {
  if (P->placed >= 0 && P->placements[P->placed].main == main) return P->placements[P->placed];
  for (size_t k = 0; k < P->placements.size(); ++k)
    if (P->placements[k].main == main) { P->placed = (int)k; return P->placements[k]; }
  (void)hipDeviceSynchronize();
  hipStream_t pick[3] = {nullptr, nullptr, nullptr};
  int np = 0;
  for (size_t k = 0; np < 3; ++k) {
    if (k == P->cand.size()) {  // every candidate so far shares a queue with the caller or a pick: draw another stream
      hipStream_t c = nullptr;
      if (k >= (size_t)Plan::MAXCAND || hipStreamCreateWithFlags(&c, hipStreamNonBlocking) != hipSuccess) break;
      P->cand.push_back(c);
    }
    hipStream_t c = P->cand[k];
    bool ok = false;
    if (streams_concurrent(main, c, &ok) != UDET_OK || !ok) continue;
    for (int j = 0; j < np && ok; ++j) {
      bool cc = false;
      if (streams_concurrent(pick[j], c, &cc) != UDET_OK || !cc) ok = false;
    }
    if (ok) pick[np++] = c;
  }
  return set_placement(P, main, pick, np);
}
// the host pins the layout for `main`: `n` (0..3) streams it knows to sit on distinct hardware queues, distinct from main's -- no probe
int plan_pin_lanes(Plan* P, hipStream_t main, hipStream_t const* streams, int n) {
  if (n < 0 || n > 3) { set_error("plan_pin_lanes: 0..3 side streams"); return UDET_ERR_ARG; }
  for (int i = 0; i < n; ++i) {
    if (!streams[i] || streams[i] == main) { set_error("plan_pin_lanes: side streams must be non-null and differ from the caller's"); return UDET_ERR_ARG; }
    for (int j = 0; j < i; ++j)
      if (streams[j] == streams[i]) { set_error("plan_pin_lanes: duplicate side stream"); return UDET_ERR_ARG; }
  }
  set_placement(P, main, streams, n);
  return UDET_OK;
}
Lane lane_of(Plan* P, hipStream_t main, int i) {
  if (i == 0 || !P->concurrent || P->profiling) return Lane{main, 0};
  return Lane{place_lanes(P, main).lane[i], i};
}
int plan_lane_queues(Plan* P, hipStream_t s, int* queue) {
  if (!P->concurrent) {  // every lane is the caller's stream
    for (int i = 0; i < Plan::NLANE; ++i) queue[i] = 0;
    return 1;
  }
  const Plan::Placement& pl = place_lanes(P, s);
  for (int i = 0; i < Plan::NLANE; ++i) queue[i] = pl.queue[i];
  return pl.nqueues;
}
hipEvent_t next_event(Plan* P) {
  std::vector<hipEvent_t>& pool = P->in_prefetch ? P->ev_pool_prefetch : P->ev_pool;
  size_t& nx = P->in_prefetch ? P->ev_next_prefetch : P->ev_next;
  if (nx == pool.size()) {
    hipEvent_t e;
    (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    pool.push_back(e);
  }
  return pool[nx++];
}
void order_after(Plan* P, const Lane& from, const Lane& to) {
  if (from.s == to.s) return;
  hipEvent_t e = next_event(P);
  (void)hipEventRecord(e, from.s);
  (void)hipStreamWaitEvent(to.s, e, 0);
}

}  // namespace udet
