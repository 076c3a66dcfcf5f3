// ksim_sweep_rt.cpp — host side of the scenario sweep: ksim_sweep (include/ksim.h),
// ksim_sweep_nodes, ksim_sweep_explain (include/ksim_whatif.h), ksim_sweep_drain
// (include/ksim_drain.h), ksim_sweep_affinity (include/ksim_affsweep.h), ksim_sweep_volumes
// (include/ksim_volsweep.h) and ksim_sweep_policy (include/ksim_polsweep.h).
//
// Three forms share one driver: the tree form (ksim_tree.hip) and the scan form (ksim_sweep_kernel)
// for resource-only ranges, the general form (ksim_sweep_general_kernel) for every other.  A form
// states its per-scenario byte estimate, writes its scratch layout once (ksim_sweep_plan.h) and runs
// its launches; the chunk rule, the scratch (re)allocation, the weight checks, the per-chunk copies
// and the statistics are written once, below.  The general form decides once which per-scenario state
// a sweep owns (SwgPlan, with ksim_sweep_admit.h for what table facts decide) and runs in steps over it.
#include "ksim_handle.h"
#include "ksim_polsweep_rules.h"
#include "ksim_sweep_admit.h"
#include "ksim_sweep_plan.h"

#include "../../include/ksim_affsweep.h"
#include "../../include/ksim_drain.h"
#include "../../include/ksim_polsweep.h"
#include "../../include/ksim_volsweep.h"
#include "../../include/ksim_whatif.h"

// ksim_sweep_policy.hip: a chunk's outcome records, [n_scen][KSIM_SWEEP_OUTCOME_WORDS], behind its sweep
// kernel on the stream; ev1 is recorded again behind it
extern "C" hipError_t ksim_sweep_outcome_launch(const KsimCtx* ctx, int32_t n_scen, int32_t* out, hipEvent_t ev1,
                                                hipStream_t st);

namespace {

// device bytes of one scenario's records: [cap] pod indices + [cap][KSIM_NREASONS] histograms
size_t why_bytes(int32_t cap) { return (size_t)cap * (1 + KSIM_NREASONS) * 4; }

// One sweep call, as every form reads it.  absent: [n_scen][aw] words, a set bit = the node is not
// listed in that scenario; weights NULL = the handle's own; rq (ksim_sweep_drain): every scenario's
// prefix queue, scheduled before the range (count may then be 0).
struct Sweep {
  ksim_handle* h = nullptr;
  const char* who = "";
  const int64_t* weights = nullptr;
  const uint32_t* absent = nullptr;
  int32_t n_scen = 0;
  int64_t first = 0, count = 0;
  int32_t* out_node = nullptr;
  uint64_t* out_counters = nullptr;
  int32_t* out_scheduled = nullptr;
  const ksim_sweep_failures* fail = nullptr;
  ksim_stats* st = nullptr;
  const ksim_sweep_requeue* rq = nullptr;
  int32_t* out_rehosted = nullptr;
  int32_t aw = 0;    // node-set words per scenario
  int32_t wcap = 0;  // records of failed pods a scenario keeps on the device (0: none)
  // ksim_sweep_affinity: the tables' inter-pod affinity terms are swept (the IPA instantiations), every
  // scenario's counts less the residents on its absent nodes (res may be null: nothing is corrected)
  bool ipa = false;
  const ksim_sweep_residents* res = nullptr;
  // ksim_sweep_volumes: range and prefix pods may mount volumes (the VOL instantiations), every scenario
  // on its own copy of the mounts; affinity terms in the tables are swept as by ksim_sweep_affinity
  bool vol = false;
  // ksim_sweep_policy: weights holds whole rows, [n_scen][KSIM_NW], checked by the entry
  // (ksim_policy_weight_rules); the queue takes whichever instantiation it would without weights (the
  // VOL ones when volume tables are loaded), and outcome (may be null) receives every scenario's record
  bool pol = false;
  const ksim_sweep_outcome* outcome = nullptr;

  size_t S() const { return (size_t)n_scen; }
  size_t P() const { return (size_t)count; }
  size_t T() const { return rq ? (size_t)rq->off[n_scen] : 0; }  // prefix pods of all scenarios
  size_t MW() const { return absent ? (size_t)aw * 4 : 0; }      // bytes of a scenario's node set
  // Records a scenario keeps: none without a record array, and never more than its queue has pods.
  void set_wcap(int64_t queue) { wcap = fail && fail->cap > 0 ? (int32_t)std::min<int64_t>(fail->cap, queue) : 0; }
};

// A chunk's outputs on the device, in every form: placements [C][count], counters [C], the chunk's
// slice of the node sets, the records of failed pods, and (general form) the prefix answers.
struct SweepOut {
  int32_t* node;
  uint64_t* counter;
  uint32_t* absent;
  int32_t *why_pod, *why_hist;
  int32_t* pre;
  int32_t* outcome;  // [C][KSIM_SWEEP_OUTCOME_WORDS] (ksim_sweep_policy with outcome records)
};

SweepOut carve_out(KsimSweepCarver& cv, size_t C, const Sweep& sw) {
  SweepOut o{};
  o.node = cv.take<int32_t>(C * sw.P());
  o.counter = cv.take<uint64_t>(C);
  if (sw.absent) o.absent = cv.take<uint32_t>(C * (size_t)sw.aw);
  if (sw.wcap) {
    o.why_pod = cv.take<int32_t>(C * (size_t)sw.wcap);
    o.why_hist = cv.take<int32_t>(C * (size_t)sw.wcap * KSIM_NREASONS);
  }
  if (sw.outcome) o.outcome = cv.take<int32_t>(C * KSIM_SWEEP_OUTCOME_WORDS);
  return o;
}

// The chunk of a sweep and its scratch.  The chunk: at most 24 GiB (all 4,096 C5 scenarios, ~3.7 MB
// each, in one launch) and at most half of the device memory free now (a shared or smaller device
// gets smaller chunks), less the form's chunk-independent bytes, at `per` bytes a scenario;
// KSIM_SWEEP_CHUNK caps it (tests).  The slot is reused when it holds the layout at that chunk; else
// it is replaced, and an allocation that fails halves the chunk until one fits.  layout(carver, C)
// is then run over the slot.  Returns the chunk; 0 after KSIM_E_NOMEM (one scenario does not fit).
template <class Layout>
int32_t sweep_scratch(const Sweep& sw, void** slot, size_t* slot_bytes, size_t per, size_t fixed, Layout layout) {
  ksim_handle* h = sw.h;
  size_t budget = (size_t)24 << 30, mfree = 0, mtotal = 0;
  if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess && mfree / 2 < budget) budget = mfree / 2;
  budget = budget > fixed ? budget - fixed : 0;
  const char* ch = getenv("KSIM_SWEEP_CHUNK");
  const int cap = ch ? atoi(ch) : 0;
  int32_t chunk = ksim_sweep_chunk(sw.S(), budget, per, ch ? &cap : nullptr);
  if (*slot_bytes < ksim_sweep_measure(layout, (size_t)chunk)) {
    if (*slot) {
      for (auto& b : h->bufs)
        if (b.p == *slot) b.p = nullptr;
      (void)hipFree(*slot);
      *slot = nullptr;
      *slot_bytes = 0;
    }
    for (;; chunk = ksim_sweep_halve(chunk)) {
      const size_t need = ksim_sweep_measure(layout, (size_t)chunk);
      void* p = nullptr;
      if (hipMalloc(&p, need) == hipSuccess) {
        h->bufs.push_back({p, need});
        *slot = p;
        *slot_bytes = need;
        break;
      }
      (void)hipGetLastError();
      if (chunk == 1) {
        ksim_fail(h, KSIM_E_NOMEM, "%s: no device memory for one scenario (%zu bytes)", sw.who, need);
        return 0;
      }
    }
  }
  KsimSweepCarver cv(*slot);
  layout(cv, (size_t)chunk);
  return chunk;
}

// Every scenario's map weights as [n_scen][3] (LeastRequested, MostRequested, Balanced; the handle's
// own without scenario weights), checked against the form's packed score: each weight, and their sum
// with `wspr` (the spread weight a spread pod's score carries beside them), at most wmax.
int sweep_weights(const Sweep& sw, int64_t wspr, int64_t wmax, const char* scores, int bits, std::vector<int64_t>* w3) {
  ksim_handle* h = sw.h;
  w3->assign(sw.S() * 3, 0);
  for (int32_t sidx = 0; sidx < sw.n_scen; ++sidx) {
    const int64_t* w = sw.weights ? sw.weights + (size_t)sidx * KSIM_NW : h->ctx.w;
    if (sw.weights && (w[KSIM_W_TAINT_TOLERATION] || w[KSIM_W_NODE_AFFINITY]))
      return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: scenario %d: reduce priorities are not swept", sw.who, sidx);
    if (wspr < 0 || wspr > wmax)
      return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: scenario %d: weight out of range", sw.who, sidx);
    int64_t tot = wspr, *row = w3->data() + 3 * (size_t)sidx;
    for (int k : {KSIM_W_LEAST_REQUESTED, KSIM_W_MOST_REQUESTED, KSIM_W_BALANCED}) {
      if (w[k] < 0 || w[k] > wmax)
        return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: scenario %d: weight out of range", sw.who, sidx);
      tot += w[k];
      *row++ = w[k];
    }
    if (tot > wmax)
      return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: scenario %d: %s exceed %d bits", sw.who, sidx, scores, bits);
  }
  return KSIM_OK;
}

// failed pods of scenario s's prefix queue (ksim_sweep_drain; none without one)
int64_t pre_failed(const ksim_sweep_requeue* rq, int32_t s) {
  int64_t nf = 0;
  for (int64_t k = rq ? rq->off[s] : 0; rq && k < rq->off[s + 1]; ++k) nf += rq->out_node[k] < 0;
  return nf;
}

// A chunk's records ([nsc][cap] pods, [nsc][cap][KSIM_NREASONS] histograms on the device) into the
// caller's arrays at the chunk's scenario offset s0: per scenario the first min(failed, cap), the
// words past them left unwritten.  The chunk's placements and prefix answers are already on the host.
int why_copy_out(const Sweep& sw, const SweepOut& d, int32_t s0, int32_t nsc) {
  ksim_handle* h = sw.h;
  const ksim_sweep_failures* fail = sw.fail;
  const int32_t cap = sw.wcap;
  const int64_t count = sw.count;
  if (!cap) return KSIM_OK;
  const int32_t* out_node = sw.out_node + (size_t)s0 * sw.P();
  std::vector<int32_t> kept((size_t)nsc);
  size_t total = 0;
  for (int32_t s = 0; s < nsc; ++s) {
    int64_t nf = pre_failed(sw.rq, s0 + s);
    for (int64_t k = 0; k < count; ++k) nf += out_node[(size_t)s * count + k] < 0;
    kept[s] = (int32_t)std::min<int64_t>(nf, cap);
    total += (size_t)kept[s];
  }
  if (!total) return KSIM_OK;
  const size_t ucap = (size_t)fail->cap;  // the caller's stride
  // few kept records in a large chunk: one copy per scenario; else the chunk's arrays in one go
  const bool whole = total * 4 >= (size_t)nsc * cap || (size_t)nsc * why_bytes(cap) <= ((size_t)8 << 20);
  std::vector<int32_t> hp, hh;
  if (whole) {
    hp.resize((size_t)nsc * cap);
    hh.resize((size_t)nsc * cap * KSIM_NREASONS);
    HIPCHK(h, hipMemcpy(hp.data(), d.why_pod, hp.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(hh.data(), d.why_hist, hh.size() * 4, hipMemcpyDeviceToHost));
  }
  for (int32_t s = 0; s < nsc; ++s) {
    const size_t k = (size_t)kept[s];
    if (!k) continue;
    int32_t* up = fail->pod + (size_t)(s0 + s) * ucap;
    int32_t* uh = fail->hist + (size_t)(s0 + s) * ucap * KSIM_NREASONS;
    if (whole) {
      memcpy(up, hp.data() + (size_t)s * cap, k * 4);
      memcpy(uh, hh.data() + (size_t)s * cap * KSIM_NREASONS, k * KSIM_NREASONS * 4);
    } else {
      HIPCHK(h, hipMemcpy(up, d.why_pod + (size_t)s * cap, k * 4, hipMemcpyDeviceToHost));
      HIPCHK(h, hipMemcpy(uh, d.why_hist + (size_t)s * cap * KSIM_NREASONS, k * KSIM_NREASONS * 4,
                          hipMemcpyDeviceToHost));
    }
  }
  return KSIM_OK;
}

// Before a chunk's launch: its slice of the node sets.
int chunk_absent(const Sweep& sw, const SweepOut& d, int32_t s0, int32_t nsc) {
  if (sw.absent)
    HIPCHK(sw.h, hipMemcpyAsync(d.absent, sw.absent + (size_t)s0 * sw.aw, (size_t)nsc * sw.MW(), hipMemcpyHostToDevice,
                                ksim_stream(sw.h)));
  return KSIM_OK;
}

// After a chunk's launch has ended: placements, counters, prefix answers and explain records into
// the caller's arrays at the chunk's scenario offset s0.
int chunk_out(const Sweep& sw, const SweepOut& d, int32_t s0, int32_t nsc) {
  ksim_handle* h = sw.h;
  const size_t P = sw.P();
  const ksim_sweep_requeue* rq = sw.rq;
  if (P) HIPCHK(h, hipMemcpy(sw.out_node + (size_t)s0 * P, d.node, (size_t)nsc * P * 4, hipMemcpyDeviceToHost));
  if (sw.out_counters) HIPCHK(h, hipMemcpy(sw.out_counters + s0, d.counter, (size_t)nsc * 8, hipMemcpyDeviceToHost));
  if (rq && rq->off[s0 + nsc] > rq->off[s0])
    HIPCHK(h, hipMemcpy(rq->out_node + rq->off[s0], d.pre + rq->off[s0], (size_t)(rq->off[s0 + nsc] - rq->off[s0]) * 4,
                        hipMemcpyDeviceToHost));
  if (sw.outcome) {  // the chunk's records into the caller's four arrays
    std::vector<int32_t> rec((size_t)nsc * KSIM_SWEEP_OUTCOME_WORDS);
    HIPCHK(h, hipMemcpy(rec.data(), d.outcome, rec.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t s = 0; s < nsc; ++s) {
      const int32_t* r = rec.data() + (size_t)s * KSIM_SWEEP_OUTCOME_WORDS;
      sw.outcome->listed[s0 + s] = r[0];
      sw.outcome->used[s0 + s] = r[1];
      memcpy(sw.outcome->free_cpu + (size_t)(s0 + s) * KSIM_OUTCOME_BUCKETS, r + 2, KSIM_OUTCOME_BUCKETS * 4);
      memcpy(sw.outcome->free_mem + (size_t)(s0 + s) * KSIM_OUTCOME_BUCKETS, r + 2 + KSIM_OUTCOME_BUCKETS,
             KSIM_OUTCOME_BUCKETS * 4);
    }
  }
  return why_copy_out(sw, d, s0, nsc);
}

// After the last chunk: the statistics block and the per-scenario counts every entry point returns
// (pods bound, prefix pods re-hosted, failed pods, nodes listed).
void sweep_done(const Sweep& sw, int32_t chunk, int32_t mode, float device_ms, float kernel_ms) {
  const int64_t n = sw.h->ctx.n, count = sw.count;
  const size_t SP = sw.S() * sw.P(), T = sw.T();
  if (ksim_stats* st = sw.st) {
    memset(st, 0, sizeof *st);
    st->pods = (int64_t)(SP + T);
    int64_t b = 0;
    for (size_t k = 0; k < SP; ++k) b += sw.out_node[k] >= 0;
    for (size_t k = 0; k < T; ++k) b += sw.rq->out_node[k] >= 0;
    st->scheduled = b;
    st->node_evals = (int64_t)(SP + T) * n;
    st->device_ms = device_ms;
    st->kernel_ms = kernel_ms;
    st->kernel_launches = (sw.n_scen + chunk - 1) / chunk;
    st->mode = mode;
    st->blocks = chunk;
  }
  if (!sw.out_scheduled && !sw.out_rehosted && !sw.fail) return;  // (4,096 x 5,000 placements not walked for nothing)
  const int32_t aw = (int32_t)((n + 31) / 32);
  for (int32_t s = 0; s < sw.n_scen; ++s) {
    int32_t bound = 0;
    for (int64_t k = 0; k < count; ++k) bound += sw.out_node[(size_t)s * count + k] >= 0;
    if (sw.out_scheduled) sw.out_scheduled[s] = bound;
    if (sw.out_rehosted) sw.out_rehosted[s] = (int32_t)(sw.rq->off[s + 1] - sw.rq->off[s] - pre_failed(sw.rq, s));
    if (!sw.fail) continue;
    if (sw.fail->count) sw.fail->count[s] = (int32_t)(pre_failed(sw.rq, s) + count - bound);
    if (sw.fail->listed) {  // n - |absent set of s| (bits at or above n ignored)
      int64_t gone = 0;
      for (int32_t w = 0; sw.absent && w < aw; ++w) {
        uint32_t m = sw.absent[(size_t)s * aw + w];
        if (w == aw - 1 && (n & 31)) m &= (1u << (n & 31)) - 1u;
        gone += __builtin_popcount(m);
      }
      sw.fail->listed[s] = (int32_t)(n - gone);
    }
  }
}

// ---- The general form of the sweep (ksim_sweep_general_kernel): a range with a pod that is not
// resource-only, or prefix queues (sw.rq, which the entry has checked).  Five steps over one plan:
// admit (the plan or the refusal), layout, upload, run, verdict.

// Which per-scenario state this sweep owns and what its packed score carries.  swg_admit decides it
// once; the layout, the uploads, the launch description and the verdict read nothing else.
struct SwgPlan {
  bool spr = false;  // a scenario's copy of the counted pairs and its affinity descriptor (the SPR instantiations)
  bool ipa = false;  // ... its carried terms and raw priority sums, and the residents (the IPA instantiations)
  bool vol = false;  // ... its mount words, slot counts and volume descriptor (the VOL instantiations)
  bool pol = false;  // every scenario's whole weight row, checked by the entry (ksim_sweep_policy)
  // the spread / inter-pod weight a pod's packed score carries beside the map weights
  int64_t wspr = 0, wipa = 0;
  size_t CL = 0, KL = 0, R = 0, VS = 0;  // words of a scenario's counted pairs / carried terms, residents, volume slots
  std::vector<int64_t> w3;               // [S][3] map weights (not pol)
};

// The messages of ksim_sweep_admit.h's codes.  A table-level refusal takes (who, zones, zone cap); a spread
// bar is the " (why)" behind the refusal of a queue pod with affinity or spread state and takes (zones, zone cap).
const char* const SWG_REFUSAL[] = {nullptr,
    "%s: no volume tables are loaded (ksim_sweep_nodes, ksim_sweep_drain and ksim_sweep_affinity sweep such a queue)",
    "%s: no affinity tables are loaded (ksim_sweep_nodes and ksim_sweep_drain sweep such a queue)",
    "%s: %d zones exceed the %d zones of a swept SelectorSpread queue (an affinity class has a spread pair)"};
const char* const SWG_SPREAD_BAR[] = {
    "", " (the tables hold inter-pod affinity terms: only SelectorSpread state is swept)",
    " (auxiliary spreading priority or lender tables are loaded)",
    " (%d zones exceed the %d zones of a swept SelectorSpread queue)"};

// Admit: the plan of this sweep, or its refusal.  Table-level refusals first (ksim_sweep_admit.h decides
// them and which state is owned, from table facts alone), then the range, then the sorted distinct prefix
// pods, then the weights.  A pod with affinity state is swept when that state is SelectorSpread's alone or
// the sweep owns the inter-pod terms (k.spread_bar open); a pod that mounts volumes when it owns the mounts.
int swg_admit(const Sweep& sw, SwgPlan* p) {
  ksim_handle* h = sw.h;
  const char* who = sw.who;
  const KsimCtx& c = h->ctx;
  const int64_t first = sw.first, count = sw.count;
  if (h->shard.world > 1) return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: a node-sharded handle sweeps resource-only pods only", who);
  if (c.n > KSIM_SWEEP_GENERAL_MAX_NODES)
    return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: %lld nodes exceed the %d-node scenario layout of pods that are not "
                                       "resource-only", who, (long long)c.n, KSIM_SWEEP_GENERAL_MAX_NODES);
  KsimSweepFacts f{};
  f.have_aff = h->have_aff; f.have_vol = h->have_vol; f.launch_tables = ksim_rt_launch_tables(h);
  f.n_carry = h->aff_n_carry; f.max_req = h->pg_max_req; f.max_pref = h->pg_max_pref; f.max_car = h->pg_max_car;
  f.n_zone = h->aff_n_zone; f.max_zones = KSIM_SWEEP_SPREAD_MAX_ZONES; f.any_spread = h->aff_any_spread;
  f.ipa = sw.ipa; f.vol = sw.vol; f.pol = sw.pol;
  const KsimSweepKind k = ksim_sweep_admit_tables(f);
  if (k.refusal)
    return ksim_fail(h, KSIM_E_UNSUPPORTED, SWG_REFUSAL[k.refusal], who, h->aff_n_zone, KSIM_SWEEP_SPREAD_MAX_ZONES);
  char spr_no[96];
  snprintf(spr_no, sizeof spr_no, SWG_SPREAD_BAR[k.spread_bar], h->aff_n_zone, KSIM_SWEEP_SPREAD_MAX_ZONES);
  p->spr = k.ipa || ksim_rt_aff_count(h, first, count) > 0;
  if (p->spr && spr_no[0])
    return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: a pod in the range carries inter-pod affinity or spread state%s", who, spr_no);
  for (int64_t q = first; !k.vol && q < first + count; ++q)
    if (h->q_vclass[q]) return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: pod %lld mounts volumes", who, (long long)q);
  if (ksim_rt_launch_tables(h))
    return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: an auxiliary spreading priority or CheckServiceAffinity's lender table is "
                                       "loaded", who);
  if (ksim_rt_range_wide(h, first, count))
    return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: a pod class in the range has more than %d reduce classes", who,
                KSIM_MAX_RCLASS);
  if (sw.T()) {  // the same refusals for the sorted distinct prefix pods
    std::vector<int64_t> idx(sw.rq->pod, sw.rq->pod + sw.T());
    std::sort(idx.begin(), idx.end());
    idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
    for (int64_t q : idx) {
      if (ksim_rt_aff_count(h, q, 1)) {
        if (spr_no[0])
          return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: re-queued pod %lld carries inter-pod affinity or spread state%s", who,
                      (long long)q, spr_no);
        p->spr = true;
      }
      if (!k.vol && h->q_vclass[q])
        return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: re-queued pod %lld mounts volumes", who, (long long)q);
      if (ksim_rt_range_wide(h, q, 1))
        return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: the class of re-queued pod %lld has more than %d reduce classes", who,
                    (long long)q, KSIM_MAX_RCLASS);
    }
  }
  p->ipa = k.ipa; p->vol = k.vol; p->pol = sw.pol;
  if (sw.weights && !sw.pol && (c.w[KSIM_W_TAINT_TOLERATION] || c.w[KSIM_W_NODE_AFFINITY] || c.use_na))
    return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: scenario weights over pods that are not resource-only would drop the "
                                       "handle's reduce priorities or NodePreferAvoidPods addend (weights = NULL sweeps "
                                       "under the whole configured policy)", who);
  p->wspr = (p->spr && !c.no_prio) ? c.w[KSIM_W_SELECTOR_SPREAD] : 0;
  if (sw.weights && !sw.pol && p->wspr)
    return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: scenario weights over a SelectorSpread queue would drop the handle's "
                                       "spread priority (weights = NULL sweeps under the whole configured policy)", who);
  p->wipa = (p->ipa && !c.no_prio) ? c.w[KSIM_W_INTERPOD_AFFINITY] : 0;
  p->CL = p->spr ? (size_t)h->aff_cnt_len : 0; p->KL = p->ipa ? (size_t)h->aff_carried_len : 0;
  p->R = p->ipa && sw.res ? (size_t)sw.res->n : 0; p->VS = p->vol ? (size_t)h->vol_h.vol_slots : 0;
  // a packed evaluation holds the map score (and a pod's spread and inter-pod scores) in
  // KSIM_SWEEP_GENERAL_SCORE_BITS bits: 10 x (LeastRequested + MostRequested + Balanced + spread weight
  // + inter-pod weight)
  // (ksim_sweep_policy: every scenario's own five weights, checked by the entry)
  if (p->pol) return KSIM_OK;
  return sweep_weights(sw, p->wspr + p->wipa, ((int64_t)1 << KSIM_SWEEP_GENERAL_SCORE_BITS) / 10 - 1,
                       p->ipa ? "map, spread and inter-pod scores" : "map scores", KSIM_SWEEP_GENERAL_SCORE_BITS, &p->w3);
}

// The device arrays of a general sweep, as swg_layout hands them out, and the launch arguments over them.
struct SwgScratch {
  SwgCols cols{};
  SwgArgsPre a{};
  SwgSpread sprd{}; SwgAffinity affd{}; SwgVolumes vold{};  // the feature parts of a launch (SwgLaunch)
  SweepOut d{};
  // ksim_commit's port-slot overflow bit, and the mount commit's (the handle's word is not written)
  int32_t *err = nullptr, *rnode = nullptr, *rident = nullptr, *rclass = nullptr;
  int64_t *w = nullptr, *off = nullptr, *pod = nullptr;
};

// Layout: a chunk of C scenarios' copies of every column a commit writes, their contexts and outputs,
// every scenario's weights (whole rows for ksim_sweep_policy) and the sweep's error word; then, by the
// plan, the state a scenario owns.  A new per-scenario state is one field of SwgPlan, its take()s here,
// and its init kernel in ksim_sweep_general_launch.  One chunk is one launch.  The arrays without a C are
// the whole sweep's, uploaded once: the weights, the prefix queues (off, pod, out_pre, indexed by global
// scenario), the residents and the word for the scenario whose corrected counts are negative.
void swg_layout(KsimSweepCarver& cv, size_t C, const Sweep& sw, const SwgPlan& p, SwgScratch& m) {
  const size_t N = (size_t)sw.h->ctx.n, NS = (size_t)sw.h->ctx.n_scalar, NP = (size_t)sw.h->ctx.port_slots;
  SwgCols& cols = m.cols;
  cols.req_cpu = cv.take<int64_t>(C * N); cols.req_mem = cv.take<int64_t>(C * N);
  cols.req_gpu = cv.take<int64_t>(C * N); cols.req_eph = cv.take<int64_t>(C * N);
  cols.nz_cpu = cv.take<int64_t>(C * N); cols.nz_mem = cv.take<int64_t>(C * N);
  cols.pod_count = cv.take<int32_t>(C * N); cols.port_count = cv.take<int32_t>(C * N);
  cols.flags = cv.take<uint32_t>(C * N);
  cols.req_scalar = cv.take<int64_t>(C * N * NS);
  cols.ports = cv.take<uint64_t>(C * N * NP);
  m.a.ctx = cv.take<KsimCtx>(C);
  if (sw.weights) m.w = cv.take<int64_t>(sw.S() * (p.pol ? KSIM_NW : 3));
  m.err = cv.take<int32_t>(1);
  m.d = carve_out(cv, C, sw);
  if (sw.rq) {
    m.off = cv.take<int64_t>(sw.S() + 1);
    m.pod = cv.take<int64_t>(sw.T());
    m.d.pre = cv.take<int32_t>(sw.T());
  }
  if (p.spr) {
    m.sprd.cnt = cv.take<int32_t>(C * p.CL);
    m.sprd.aff = cv.take<KsimAff>(C);
  }
  if (p.ipa) {
    m.affd.carried = cv.take<int64_t>(C * p.KL);
    m.affd.raw = cv.take<int64_t>(C * N);
    m.rnode = cv.take<int32_t>(p.R); m.rident = cv.take<int32_t>(p.R); m.rclass = cv.take<int32_t>(p.R);
    m.affd.bad = cv.take<int32_t>(1);
  }
  if (p.vol) {
    m.vold.slots = cv.take<uint64_t>(C * p.VS * N);
    m.vold.slot_count = cv.take<int32_t>(C * N);
    m.vold.vol = cv.take<KsimVol>(C);
  }
}

// Upload: the launch arguments over the scratch, and the once-per-sweep copies: prefix lists, residents,
// weight rows, error word.
int swg_upload(const Sweep& sw, const SwgPlan& p, SwgScratch& m) {
  ksim_handle* h = sw.h;
  const size_t S = sw.S(), T = sw.T(), R = p.R;
  SwgArgsPre& a = m.a;
  a.n_pods = (int32_t)sw.count; a.first = sw.first;
  a.w = p.pol ? nullptr : m.w;  // (the context kernel then keeps the handle's; the policy kernel writes the rows)
  a.out_node = m.d.node; a.out_counter = m.d.counter;
  a.why = SwWhy{sw.wcap, m.d.why_pod, m.d.why_hist};
  a.off = m.off; a.pod = m.pod; a.out_pre = m.d.pre;
  if (sw.rq) {
    HIPCHK(h, hipMemcpyAsync(m.off, sw.rq->off, (S + 1) * 8, hipMemcpyHostToDevice, ksim_stream(h)));
    if (T) HIPCHK(h, hipMemcpyAsync(m.pod, sw.rq->pod, T * 8, hipMemcpyHostToDevice, ksim_stream(h)));
  }
  if (p.spr) {  // every launch copies the handle's current counts: the handle's own are only read
    m.sprd.base = h->aff_h;
    m.sprd.cnt_len = (int64_t)p.CL;
  }
  if (p.ipa) {
    m.affd.carried_len = (int64_t)p.KL;
    m.affd.res = SwgResidents{(int64_t)R, m.rnode, m.rident, m.rclass};
    const int32_t none = INT32_MAX;
    HIPCHK(h, hipMemcpyAsync(m.affd.bad, &none, 4, hipMemcpyHostToDevice, ksim_stream(h)));
    if (R) {
      HIPCHK(h, hipMemcpyAsync(m.rnode, sw.res->node, R * 4, hipMemcpyHostToDevice, ksim_stream(h)));
      HIPCHK(h, hipMemcpyAsync(m.rident, sw.res->aff_ident, R * 4, hipMemcpyHostToDevice, ksim_stream(h)));
      HIPCHK(h, hipMemcpyAsync(m.rclass, sw.res->aff_class, R * 4, hipMemcpyHostToDevice, ksim_stream(h)));
    }
  }
  if (p.vol) m.vold.base = h->vol_h;  // every launch copies the handle's current mounts: its own are only read
  HIPCHK(h, hipMemcpy(&a.counter0, h->ctx.counter, 8, hipMemcpyDeviceToHost));
  if (m.w && p.pol) HIPCHK(h, hipMemcpyAsync(m.w, sw.weights, S * KSIM_NW * 8, hipMemcpyHostToDevice, ksim_stream(h)));
  else if (m.w) HIPCHK(h, hipMemcpyAsync(m.w, p.w3.data(), S * 24, hipMemcpyHostToDevice, ksim_stream(h)));
  HIPCHK(h, hipMemsetAsync(m.err, 0, 4, ksim_stream(h)));
  return KSIM_OK;
}

// Run: the chunk loop.  The plan's flags become the launch description's feature parts here and nowhere else.
int swg_run(const Sweep& sw, const SwgPlan& p, SwgScratch& m, int32_t chunk, float* ms) {
  ksim_handle* h = sw.h;
  SwgLaunch L{};
  L.hc = &h->ctx; L.cols = &m.cols; L.args = &m.a;
  L.spr = p.spr ? &m.sprd : nullptr;
  L.ipa = p.ipa ? &m.affd : nullptr;
  L.vol = p.vol ? &m.vold : nullptr;
  L.polw = p.pol ? m.w : nullptr;
  L.absent = m.d.absent; L.absent_words = sw.aw;
  L.err = m.err; L.ev0 = h->ev0; L.ev1 = h->ev1;
  for (int32_t s0 = 0; s0 < sw.n_scen; s0 += chunk) {
    const int32_t nsc = std::min(chunk, sw.n_scen - s0);
    m.a.scen0 = s0;  // the chunk's first scenario: its row of the weights
    L.n_scen = nsc;
    if (int rc = chunk_absent(sw, m.d, s0, nsc)) return rc;
    L.st = ksim_stream(h);
    hipError_t e = ksim_sweep_general_launch(&L);
    if (e != hipSuccess) return ksim_fail(h, KSIM_E_DEVICE, "sweep launch: %s", hipGetErrorString(e));
    if (sw.outcome) {  // the scenarios' final state, before the next chunk reuses the copies
      e = ksim_sweep_outcome_launch(m.a.ctx, nsc, m.d.outcome, h->ev1, ksim_stream(h));
      if (e != hipSuccess) return ksim_fail(h, KSIM_E_DEVICE, "sweep outcome launch: %s", hipGetErrorString(e));
    }
    HIPCHK(h, hipEventSynchronize(h->ev1));
    float c_ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&c_ms, h->ev0, h->ev1));
    *ms += c_ms;
    if (int rc = chunk_out(sw, m.d, s0, nsc)) return rc;
  }
  return KSIM_OK;
}

// Verdict: the sweep's error word, after the last chunk.
int swg_verdict(const Sweep& sw, const SwgPlan& p, const SwgScratch& m) {
  ksim_handle* h = sw.h;
  int32_t err = 0;
  HIPCHK(h, hipMemcpy(&err, m.err, 4, hipMemcpyDeviceToHost));
  if (err & KSIM_SWEEP_ERR_COUNTS) {
    int32_t bad = 0;
    HIPCHK(h, hipMemcpy(&bad, m.affd.bad, 4, hipMemcpyDeviceToHost));
    return ksim_fail(h, KSIM_E_INVAL, "%s: scenario %d: a counted pair is negative once the residents of its absent nodes "
                                 "are taken out (the residents are not the placed pods behind the handle's counts)",
                     sw.who, bad);
  }
  if (err && p.vol)
    return ksim_fail(h, KSIM_E_OVERFLOW, "%s: a node's volume slots or host-port slots overflowed, or a mount count of a "
                                    "volume saturated, in a scenario (load the volume tables with more vol_slots, or the "
                                    "node table with more port slots)", sw.who);
  if (err)
    return ksim_fail(h, KSIM_E_OVERFLOW, "%s: a node's host-port slots overflowed in a scenario (load the node table with "
                                    "more port slots)", sw.who);
  return KSIM_OK;
}

int sweep_general(Sweep& sw) {
  int64_t mmax = 0;
  for (int32_t s = 0; sw.rq && s < sw.n_scen; ++s) mmax = std::max(mmax, sw.rq->off[s + 1] - sw.rq->off[s]);
  sw.set_wcap(mmax + sw.count);  // over the longest scenario queue
  SwgPlan p;
  if (int rc = swg_admit(sw, &p)) return rc;
  SwgScratch m;
  auto layout = [&](KsimSweepCarver& cv, size_t C) { swg_layout(cv, C, sw, p, m); };
  // From the layout itself: no scenario's arrays are the chunk-independent bytes, off the budget first; 256
  // scenarios' arrays end on the carver's alignment, so the difference to none holds no padding and is a
  // scenario's bytes.
  constexpr size_t A = KsimSweepCarver::ALIGN;
  const size_t fixed = ksim_sweep_measure(layout, 0), per = (ksim_sweep_measure(layout, A) - fixed) / A;
  const int32_t chunk = sweep_scratch(sw, &sw.h->sw_scratch, &sw.h->sw_scratch_bytes, per, fixed, layout);
  if (!chunk) return KSIM_E_NOMEM;
  float ms = 0.f;
  if (int rc = swg_upload(sw, p, m)) return rc;
  if (int rc = swg_run(sw, p, m, chunk, &ms)) return rc;
  if (int rc = swg_verdict(sw, p, m)) return rc;
  sweep_done(sw, chunk, KSIM_MODE_PERSISTENT, ms, ms);
  return KSIM_OK;
}

// Tree form (ksim_tree.hip): one tree-mode wave per scenario, scenarios spread over the CUs.
int sweep_tree(const Sweep& sw, const KsimTreeGeo& g, const std::vector<int64_t>& w3) {
  ksim_handle* h = sw.h;
  KsimCtx& c = h->ctx;
  const int64_t n = c.n;
  const int32_t n_scen = sw.n_scen;
  if (!h->t_y)
    if (int rc = dev_alloc(h, &h->t_y, (size_t)2 * n)) return rc;
  const size_t N = (size_t)n, P = sw.P(), K = (size_t)g.K;
  KsimTreeSweep tsw{};
  SweepOut d{};
  int32_t *leaves = nullptr, *fitc = nullptr;
  uint64_t* levels = nullptr;
  kf64::EvCfg* dcfg = nullptr;
  auto layout = [&](KsimSweepCarver& cv, size_t C) {
    tsw.rc = cv.take<int64_t>(C * N); tsw.rm = cv.take<int64_t>(C * N);
    tsw.zc = cv.take<int64_t>(C * N); tsw.zm = cv.take<int64_t>(C * N);
    tsw.count = cv.take<int32_t>(C * N);
    leaves = cv.take<int32_t>(C * K * g.st[0]);
    levels = cv.take<uint64_t>(C * g.level_entries);
    fitc = cv.take<int32_t>(C * K);
    dcfg = cv.take<kf64::EvCfg>(C);
    d = carve_out(cv, C, sw);
    cv.take<char>(4096);  // spare past the last array: the tree kernels are not shown never to read past it
  };
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t per = al(4 * N * 8) + al(N * 4) + al(K * g.st[0] * 4) + al(g.level_entries * 8) + al(K * 4) + al(8) +
                     al(P * 4) + al(sizeof(kf64::EvCfg)) + (sw.MW() ? al(sw.MW()) : 0) + al(why_bytes(sw.wcap));
  const int32_t chunk = sweep_scratch(sw, &h->swt_scratch, &h->swt_bytes, per, 0, layout);
  if (!chunk) return KSIM_E_NOMEM;
  tsw.count_pods = sw.count;
  tsw.counter = d.counter;
  tsw.out_node = d.node;
  tsw.cfg = dcfg;
  tsw.why_cap = sw.wcap;
  tsw.why_pod = d.why_pod;
  tsw.why_hist = d.why_hist;
  std::vector<kf64::EvCfg> cfgs((size_t)n_scen);
  for (int32_t sidx = 0; sidx < n_scen; ++sidx)
    cfgs[sidx] = kf64::make_evcfg(c.preds, c.no_prio != 0, (int32_t)w3[3 * sidx], (int32_t)w3[3 * sidx + 1],
                                  (int32_t)w3[3 * sidx + 2]);
  // the kernels read the range from the handle's context: put back on every way out
  struct Range {
    KsimCtx& c;
    const int64_t first, end;
    ~Range() { c.first = first; c.end = end; }
  } saved{c, c.first, c.end};
  c.first = sw.first;
  c.end = sw.first + sw.count;
  float kms = 0.f, dms = 0.f;
  int32_t err0 = 0;
  HIPCHK(h, hipMemcpy(&err0, c.err, 4, hipMemcpyDeviceToHost));
  for (int32_t s0 = 0; s0 < n_scen; s0 += chunk) {
    tsw.nsc = std::min(chunk, n_scen - s0);
    HIPCHK(h, hipMemcpyAsync(dcfg, cfgs.data() + s0, tsw.nsc * sizeof(kf64::EvCfg), hipMemcpyHostToDevice, ksim_stream(h)));
    HIPCHK(h, hipEventRecord(h->ev0, ksim_stream(h)));
    if (int rc = chunk_absent(sw, d, s0, tsw.nsc)) return rc;
    hipError_t e = ksim_tree_sweep_init(&c, &tsw, ksim_stream(h));
    if (e == hipSuccess && sw.absent) e = ksim_tree_sweep_absent(&c, &tsw, d.absent, sw.aw, ksim_stream(h));
    if (e == hipSuccess)
      e = sw.absent ? ksim_tree_build_absent(&c, &g, h->tclass, h->tcls, leaves, levels, fitc, h->t_y, &tsw, ksim_stream(h))
                    : ksim_tree_build(&c, &g, h->tclass, h->tcls, leaves, levels, fitc, h->t_y, &tsw, ksim_stream(h));
    if (e != hipSuccess) return ksim_fail(h, KSIM_E_DEVICE, "tree sweep build: %s", hipGetErrorString(e));
    HIPCHK(h, hipEventRecord(h->ev1, ksim_stream(h)));
    e = ksim_tree_launch(&c, &g, h->tclass, h->tcls, leaves, levels, fitc, h->t_y, &tsw, ksim_stream(h));
    if (e != hipSuccess) return ksim_fail(h, KSIM_E_DEVICE, "tree sweep launch: %s", hipGetErrorString(e));
    hipEvent_t ev2 = nullptr;
    HIPCHK(h, hipEventCreate(&ev2));
    HIPCHK(h, hipEventRecord(ev2, ksim_stream(h)));
    HIPCHK(h, hipEventSynchronize(ev2));
    float b_ms = 0.f, r_ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&b_ms, h->ev0, h->ev1));
    HIPCHK(h, hipEventElapsedTime(&r_ms, h->ev1, ev2));
    (void)hipEventDestroy(ev2);
    kms += r_ms;
    dms += b_ms + r_ms;
    if (int rc = chunk_out(sw, d, s0, tsw.nsc)) return rc;
  }
  int32_t err = 0;
  HIPCHK(h, hipMemcpy(&err, c.err, 4, hipMemcpyDeviceToHost));
  if (err != err0) {
    HIPCHK(h, hipMemcpy(c.err, &err0, 4, hipMemcpyHostToDevice));
    return ksim_fail(h, KSIM_E_DEVICE, "tree sweep: device consistency error 0x%x", err & ~err0);
  }
  sweep_done(sw, chunk, KSIM_MODE_TREE, dms, kms);
  return KSIM_OK;
}

// Scan form (ksim_sweep_kernel): one workgroup per scenario, its evaluations in LDS.
int sweep_scan(const Sweep& sw, const std::vector<int64_t>& w3) {
  ksim_handle* h = sw.h;
  KsimCtx& c = h->ctx;
  const int64_t n = c.n;
  const int32_t n_scen = sw.n_scen;
  if (!h->sw_dac) {
    int rc;
    if ((rc = dev_alloc(h, &h->sw_dac, n)) || (rc = dev_alloc(h, &h->sw_dam, n)) || (rc = dev_alloc(h, &h->sw_yc, n)) ||
        (rc = dev_alloc(h, &h->sw_ym, n)))
      return rc;
    hipError_t e = ksim_sweep_prepare(c.alloc_cpu, c.alloc_mem, n, h->sw_dac, h->sw_dam, h->sw_yc, h->sw_ym, ksim_stream(h));
    if (e != hipSuccess) return ksim_fail(h, KSIM_E_DEVICE, "sweep prepare: %s", hipGetErrorString(e));
  }
  // scratch: [C][n] x (4 float64 + int32) and outputs for a chunk of C scenarios, the pods and every
  // scenario's weights.  One chunk is one launch.
  const size_t S = sw.S(), N = (size_t)n, P = sw.P();
  SwArgsWhy a{};
  SweepOut d{};
  kf64::FPod* fpods = nullptr;
  int32_t* dw = nullptr;
  auto layout = [&](KsimSweepCarver& cv, size_t C) {
    a.rc = cv.take<double>(C * N); a.rm = cv.take<double>(C * N);
    a.zc = cv.take<double>(C * N); a.zm = cv.take<double>(C * N);
    a.count = cv.take<int32_t>(C * N);
    fpods = cv.take<kf64::FPod>(P);
    dw = cv.take<int32_t>(S * 3);
    d = carve_out(cv, C, sw);
  };
  const size_t per = N * 36 + P * 4 + 8 + sw.MW() + why_bytes(sw.wcap);
  const int32_t chunk = sweep_scratch(sw, &h->sw_scratch, &h->sw_scratch_bytes, per, 0, layout);
  if (!chunk) return KSIM_E_NOMEM;
  a.n = n; a.n_pods = (int32_t)sw.count;
  a.dac = h->sw_dac; a.dam = h->sw_dam; a.yc = h->sw_yc; a.ym = h->sw_ym;
  a.allowed = c.allowed_pods; a.flags = c.flags;
  a.pods = fpods;
  a.w = dw;
  a.out_node = d.node;
  a.out_counter = d.counter;
  a.why = SwWhy{sw.wcap, d.why_pod, d.why_hist};
  a.preds = c.preds; a.no_prio = c.no_prio;
  const std::vector<int32_t> w32(w3.begin(), w3.end());
  HIPCHK(h, hipMemcpy(&a.counter0, c.counter, 8, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpyAsync(dw, w32.data(), S * 12, hipMemcpyHostToDevice, ksim_stream(h)));
  float ms = 0.f;
  for (int32_t s0 = 0; s0 < n_scen; s0 += chunk) {
    const int32_t nsc = std::min(chunk, n_scen - s0);
    a.scen0 = s0;  // the chunk's first scenario: its row of the weights
    if (int rc = chunk_absent(sw, d, s0, nsc)) return rc;
    hipError_t e = ksim_sweep_launch(c.req_cpu, c.req_mem, c.nz_cpu, c.nz_mem, c.pod_count, c.pods + sw.first, fpods, &a,
                                     nsc, d.absent, sw.aw, h->ev0, h->ev1, ksim_stream(h));
    if (e != hipSuccess) return ksim_fail(h, KSIM_E_DEVICE, "sweep launch: %s", hipGetErrorString(e));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    float c_ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&c_ms, h->ev0, h->ev1));
    ms += c_ms;
    if (int rc = chunk_out(sw, d, s0, nsc)) return rc;
  }
  sweep_done(sw, chunk, KSIM_MODE_PERSISTENT, ms, ms);
  return KSIM_OK;
}

// ksim_sweep (absent = NULL, weights given), ksim_sweep_nodes and ksim_sweep_explain (fail).
int sweep_impl(Sweep sw) {
  ksim_handle* h = sw.h;
  const char* who = sw.who;
  const int64_t first = sw.first, count = sw.count;
  if (!h || !sw.out_node) return ksim_fail(h, KSIM_E_INVAL, "%s: null argument", who);
  if (!h->have_pods) return ksim_fail(h, KSIM_E_STATE, "%s: load nodes, classes and pods first", who);
  if (sw.n_scen <= 0 || first < 0 || count <= 0 || first + count > h->n_pods || count > INT32_MAX)
    return ksim_fail(h, KSIM_E_INVAL, "%s: bad scenario count or pod range", who);
  HIPCHK(h, hipSetDevice(h->device));
  KsimCtx& c = h->ctx;
  const int64_t n = c.n;
  if (n == 0) return ksim_fail(h, KSIM_E_NO_NODES, "no nodes available to schedule pods");
  if (int rc0 = ksim_rt_check_aff(h, who)) return rc0;
  sw.aw = (int32_t)((n + 31) / 32);
  // a pod that is not resource-only (ports, selectors, taints, nodeName, gpu / ephemeral / extended
  // requests, more than one reduce class): the general form; else the forms below, as ever
  if (h->fast_pre[first + count] - h->fast_pre[first] != count) return sweep_general(sw);
  if (n > KSIM_SWEEP_MAX_NODES)
    return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: %lld nodes exceed the %d-node scenario layout", who, (long long)n,
                KSIM_SWEEP_MAX_NODES);
  // weights NULL: the handle's own map weights.  Its reduce and constant priorities are the same
  // value on every node for the pods admitted above (fast_k: one reduce class) and stay out of
  // the packed score (10 x the weights' sum in 16 bits), as in the fast persistent kernel.
  std::vector<int64_t> w3;
  if (int rc = sweep_weights(sw, 0, 0xFFFF / 10, "scores", 16, &w3)) return rc;
  // float64 exactness: capacities below 2^48 (they never grow), and the requested quantities +
  // count x the largest pod quantity stay below 2^48
  {
    int64_t qmax = 0, nmax = 0, amax = 0;
    for (int64_t i = first; i < first + count; ++i) qmax = std::max(qmax, h->pod_qmax[i]);
    std::vector<int64_t> col((size_t)n);
    for (const int64_t* d : {c.alloc_cpu, c.alloc_mem, (const int64_t*)c.req_cpu, (const int64_t*)c.req_mem,
                             (const int64_t*)c.nz_cpu, (const int64_t*)c.nz_mem}) {
      HIPCHK(h, hipMemcpy(col.data(), d, (size_t)n * 8, hipMemcpyDeviceToHost));
      int64_t& mx = (d == c.alloc_cpu || d == c.alloc_mem) ? amax : nmax;
      for (int64_t v : col) mx = std::max(mx, v < 0 ? INT64_MAX / 2 : v);
    }
    const int64_t lim = (int64_t)1 << 48;
    if (amax >= lim || nmax >= lim || qmax >= lim || count > lim / std::max<int64_t>(qmax, 1) || nmax + count * qmax >= lim)
      return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: quantities may leave the exact float64 range (2^48)", who);
  }
  sw.set_wcap(count);
  if (!getenv("KSIM_SWEEP_SCAN") && h->n_tcls > 0 && n < ((int64_t)1 << 24) && !h->pfast_off) {
    KsimTreeGeo g{};
    // a small LDS plan: several scenarios' waves per CU hide each other's memory latency
    const char* lb = getenv("KSIM_SWEEP_LDS");
    if (ksim_tree_plan(n, h->n_tcls, lb ? atoll(lb) : 24 * 1024, 0, &g) || ksim_tree_plan(n, h->n_tcls, 0, 0, &g))
      return sweep_tree(sw, g, w3);
  }
  return sweep_scan(sw, w3);
}

// ksim_sweep_explain, ksim_sweep_drain: the record arrays' shape, before the handle is touched
int check_failures(ksim_handle* h, const char* who, const ksim_sweep_failures* fail) {
  if (fail && (fail->cap < 0 || (fail->cap > 0 && (!fail->pod || !fail->hist))))
    return ksim_fail(h, KSIM_E_INVAL, "%s: a negative record cap, or a cap without record arrays", who);
  return KSIM_OK;
}

// ksim_sweep_drain, ksim_sweep_affinity: the scenarios' queues (rq null: the range alone), by what needs
// no device, before the handle is touched
int check_queue(ksim_handle* h, const char* who, int32_t n_scen, const ksim_sweep_requeue* rq, bool need_rq, int64_t first,
                int64_t count, int32_t* out_node) {
  if (n_scen <= 0 || first < 0 || count < 0 || (!rq && !need_rq && (count == 0 || count > INT32_MAX)))
    return ksim_fail(h, KSIM_E_INVAL, "%s: bad scenario count or pod range", who);
  if ((need_rq && !rq) || (rq && !rq->off)) return ksim_fail(h, KSIM_E_INVAL, "%s: null re-queue lists", who);
  if (rq && rq->off[0] != 0) return ksim_fail(h, KSIM_E_INVAL, "%s: off[0] must be 0", who);
  for (int32_t s = 0; rq && s < n_scen; ++s) {
    if (rq->off[s + 1] < rq->off[s]) return ksim_fail(h, KSIM_E_INVAL, "%s: off decreases at scenario %d", who, s);
    if (rq->off[s + 1] - rq->off[s] > (int64_t)INT32_MAX - count)
      return ksim_fail(h, KSIM_E_INVAL, "%s: the queue of scenario %d exceeds INT32_MAX pods", who, s);
  }
  const int64_t T = rq ? rq->off[n_scen] : 0;
  if (T > 0 && (!rq->pod || !rq->out_node))
    return ksim_fail(h, KSIM_E_INVAL, "%s: re-queued pods without a pod or out_node array", who);
  if (T == 0 && count == 0) return ksim_fail(h, KSIM_E_INVAL, "%s: neither re-queued pods nor a pod range", who);
  if (count > 0 && !out_node) return ksim_fail(h, KSIM_E_INVAL, "%s: null argument", who);
  if (!h) return ksim_fail(h, KSIM_E_INVAL, "%s: null argument", who);
  if (!h->have_pods) return ksim_fail(h, KSIM_E_STATE, "%s: load nodes, classes and pods first", who);
  if (first + count > h->n_pods) return ksim_fail(h, KSIM_E_INVAL, "%s: bad scenario count or pod range", who);
  for (int64_t k = 0; k < T; ++k)
    if (rq->pod[k] < 0 || rq->pod[k] >= h->n_pods)
      return ksim_fail(h, KSIM_E_INVAL, "%s: re-queued pod index %lld outside the loaded queue of %lld pods", who,
                  (long long)rq->pod[k], (long long)h->n_pods);
  return KSIM_OK;
}

// ksim_sweep_affinity, ksim_sweep_volumes: stale tables, and the residents against the loaded affinity
// tables, before the device is touched
int check_residents(ksim_handle* h, const char* who, const ksim_sweep_residents* res) {
  if (h->have_aff && h->aff_stale)
    return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: the affinity tables predate a node event; load them again", who);
  if (h->have_vol && h->vol_stale)
    return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: the volume tables predate a node event; load them again", who);
  if (res && res->n < 0) return ksim_fail(h, KSIM_E_INVAL, "%s: a negative number of residents", who);
  if (res && res->n > 0) {
    if (!res->node || !res->aff_ident || !res->aff_class)
      return ksim_fail(h, KSIM_E_INVAL, "%s: residents without a node, aff_ident or aff_class array", who);
    // (without tables the call is refused below; the bounds are then the empty tables')
    const int32_t ni = h->have_aff ? h->aff_n_ident : 0, na = h->have_aff ? h->aff_n_aclass : 0;
    for (int64_t k = 0; k < res->n; ++k) {
      if (res->node[k] < 0 || res->node[k] >= h->ctx.n)
        return ksim_fail(h, KSIM_E_INVAL, "%s: resident %lld: node %d outside [0, %lld)", who, (long long)k, res->node[k],
                    (long long)h->ctx.n);
      if (res->aff_ident[k] < 0 || res->aff_ident[k] > ni || res->aff_class[k] < 0 || res->aff_class[k] > na)
        return ksim_fail(h, KSIM_E_INVAL, "%s: resident %lld: identity %d or class %d beyond the loaded tables (%d, %d)", who,
                    (long long)k, res->aff_ident[k], res->aff_class[k], ni, na);
    }
  }
  return KSIM_OK;
}

// The arguments every entry has into a Sweep; an entry names its others itself.
Sweep sweep_of(ksim_handle* h, const char* who, int32_t n_scen, int64_t first, int64_t count, int32_t* out_node,
               uint64_t* out_counters, ksim_stats* st) {
  Sweep sw;
  sw.h = h; sw.who = who; sw.n_scen = n_scen; sw.first = first; sw.count = count;
  sw.out_node = out_node; sw.out_counters = out_counters; sw.st = st;
  return sw;
}

// ksim_sweep_drain, ksim_sweep_affinity, ksim_sweep_volumes and ksim_sweep_policy: the checks they share that
// need no device, in their order.  drain (ksim_sweep_drain): the queues must be given; the others check the
// stale tables and the residents.
int queue_checks(const Sweep& sw, bool drain) {
  if (int rc = check_failures(sw.h, sw.who, sw.fail)) return rc;
  if (int rc = check_queue(sw.h, sw.who, sw.n_scen, sw.rq, drain, sw.first, sw.count, sw.out_node)) return rc;
  return drain ? KSIM_OK : check_residents(sw.h, sw.who, sw.res);
}

// ... and, once the entry has set the device, what they share before the general form.  drain: the affinity
// tables are checked as by ksim_sweep_nodes and out_rehosted is always written; the others write zeros to
// out_rehosted (may be null) when there are no queues.
int queue_sweep(Sweep& sw, bool drain) {
  ksim_handle* h = sw.h;
  if (h->ctx.n == 0) return ksim_fail(h, KSIM_E_NO_NODES, "no nodes available to schedule pods");
  if (drain)
    if (int rc0 = ksim_rt_check_aff(h, sw.who)) return rc0;
  if (!drain && !sw.rq) {
    if (sw.out_rehosted) std::fill(sw.out_rehosted, sw.out_rehosted + sw.n_scen, 0);
    sw.out_rehosted = nullptr;
  }
  sw.aw = (int32_t)((h->ctx.n + 31) / 32);
  return sweep_general(sw);
}

}  // namespace

extern "C" {

int ksim_sweep(ksim_handle* h, const int64_t* weights, int32_t n_scen, int64_t first, int64_t count, int32_t* out_node,
               uint64_t* out_counters, ksim_stats* st) {
  if (!weights) return ksim_fail(h, KSIM_E_INVAL, "ksim_sweep: null argument");
  Sweep sw = sweep_of(h, "ksim_sweep", n_scen, first, count, out_node, out_counters, st);
  sw.weights = weights;
  return sweep_impl(sw);
}

int ksim_sweep_nodes(ksim_handle* h, const int64_t* weights, const uint32_t* absent, int32_t n_scen, int64_t first,
                     int64_t count, int32_t* out_node, uint64_t* out_counters, int32_t* out_scheduled, ksim_stats* st) {
  Sweep sw = sweep_of(h, "ksim_sweep_nodes", n_scen, first, count, out_node, out_counters, st);
  sw.weights = weights; sw.absent = absent; sw.out_scheduled = out_scheduled;
  return sweep_impl(sw);
}

int ksim_sweep_explain(ksim_handle* h, const int64_t* weights, const uint32_t* absent, int32_t n_scen, int64_t first,
                       int64_t count, int32_t* out_node, uint64_t* out_counters, int32_t* out_scheduled,
                       const ksim_sweep_failures* fail, ksim_stats* st) {
  if (int rc = check_failures(h, "ksim_sweep_explain", fail)) return rc;
  Sweep sw = sweep_of(h, "ksim_sweep_explain", n_scen, first, count, out_node, out_counters, st);
  sw.weights = weights; sw.absent = absent; sw.out_scheduled = out_scheduled; sw.fail = fail;
  return sweep_impl(sw);
}

int ksim_sweep_drain(ksim_handle* h, const uint32_t* absent, int32_t n_scen, const ksim_sweep_requeue* rq, int64_t first,
                     int64_t count, int32_t* out_node, uint64_t* out_counters, int32_t* out_scheduled,
                     int32_t* out_rehosted, const ksim_sweep_failures* fail, ksim_stats* st) {
  Sweep sw = sweep_of(h, "ksim_sweep_drain", n_scen, first, count, out_node, out_counters, st);
  sw.absent = absent; sw.out_scheduled = out_scheduled; sw.fail = fail; sw.rq = rq; sw.out_rehosted = out_rehosted;
  if (int rc = queue_checks(sw, true)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return queue_sweep(sw, true);
}

int ksim_sweep_affinity(ksim_handle* h, const uint32_t* absent, int32_t n_scen, const ksim_sweep_residents* res,
                        const ksim_sweep_requeue* rq, int64_t first, int64_t count, int32_t* out_node,
                        uint64_t* out_counters, int32_t* out_scheduled, int32_t* out_rehosted,
                        const ksim_sweep_failures* fail, ksim_stats* st) {
  Sweep sw = sweep_of(h, "ksim_sweep_affinity", n_scen, first, count, out_node, out_counters, st);
  sw.absent = absent; sw.out_scheduled = out_scheduled; sw.fail = fail; sw.rq = rq; sw.out_rehosted = out_rehosted;
  sw.res = res; sw.ipa = true;
  if (int rc = queue_checks(sw, false)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return queue_sweep(sw, false);
}

int ksim_sweep_volumes(ksim_handle* h, const uint32_t* absent, int32_t n_scen, const ksim_sweep_residents* res,
                       const ksim_sweep_requeue* rq, int64_t first, int64_t count, int32_t* out_node,
                       uint64_t* out_counters, int32_t* out_scheduled, int32_t* out_rehosted,
                       const ksim_sweep_failures* fail, ksim_stats* st) {
  Sweep sw = sweep_of(h, "ksim_sweep_volumes", n_scen, first, count, out_node, out_counters, st);
  sw.absent = absent; sw.out_scheduled = out_scheduled; sw.fail = fail; sw.rq = rq; sw.out_rehosted = out_rehosted;
  sw.res = res; sw.vol = true;
  if (int rc = queue_checks(sw, false)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  return queue_sweep(sw, false);
}

int ksim_sweep_policy(ksim_handle* h, const int64_t* weights, const uint32_t* absent, int32_t n_scen,
                      const ksim_sweep_residents* res, const ksim_sweep_requeue* rq, int64_t first, int64_t count,
                      int32_t* out_node, uint64_t* out_counters, int32_t* out_scheduled, int32_t* out_rehosted,
                      const ksim_sweep_failures* fail, const ksim_sweep_outcome* outcome, ksim_stats* st) {
  const char* who = "ksim_sweep_policy";
  if (!weights) return ksim_fail(h, KSIM_E_INVAL, "%s: null argument", who);
  if (outcome && (!outcome->listed || !outcome->used || !outcome->free_cpu || !outcome->free_mem))
    return ksim_fail(h, KSIM_E_INVAL, "%s: an outcome without a listed, used, free_cpu or free_mem array", who);
  Sweep sw = sweep_of(h, who, n_scen, first, count, out_node, out_counters, st);
  sw.absent = absent; sw.out_scheduled = out_scheduled; sw.fail = fail; sw.rq = rq; sw.out_rehosted = out_rehosted;
  sw.res = res; sw.pol = true; sw.weights = weights; sw.outcome = outcome;
  if (int rc = queue_checks(sw, false)) return rc;
  {  // the weight rules, on the host alone
    int32_t s = 0;
    int slot = -1;
    switch (ksim_policy_weight_rules(h->ctx.w, h->ctx.no_prio, weights, n_scen, KSIM_SWEEP_GENERAL_SCORE_BITS, &s, &slot)) {
      case KSIM_POLICY_OK: break;
      case KSIM_POLICY_NO_PRIORITIES:
        return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: the handle has an empty prioritizer list (EqualPriority): there is no "
                                           "policy to vary", who);
      case KSIM_POLICY_RANGE:
        return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: scenario %d: weight out of range (%s is negative)", who, s,
                         ksim_policy_slot_name(slot));
      case KSIM_POLICY_RESTRICTED:
        return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: scenario %d: %s has a weight but the handle's policy has none (its "
                                           "tables were not built: a scenario rescales or drops such a priority)", who, s,
                         ksim_policy_slot_name(slot));
      case KSIM_POLICY_SCORE:
        return ksim_fail(h, KSIM_E_UNSUPPORTED, "%s: scenario %d: map, spread and inter-pod scores exceed %d bits", who, s,
                         KSIM_SWEEP_GENERAL_SCORE_BITS);
    }
  }
  HIPCHK(h, hipSetDevice(h->device));
  return queue_sweep(sw, false);
}

}  // extern "C"
