// tier1.cpp — the device half of the TFHE C API (Tier-1) over the MI355X engine.
//
// The drop-in boundary of SURVEY.md §8(b), cloud side: bootsXXX, tfhe_bootstrap_(woKS_)FFT,
// lweKeySwitch and the L1 blind-rotation entry points run on the GPU through a device context
// cached per key (engine.cpp).  The keys themselves, their generation and everything else that
// needs no device are tfhe_api.cpp; the two meet in the four functions of api_internal.h.
//
// Reentrancy: every calling thread gets its own "lane" (stream + scratch) per key, so
// OpenMP callers (Cipher.cpp:116-120, cloud.cpp:390-393) run concurrently; the reference's
// global FFT scratch (lagrangehalfc_impl.cu:4) has no counterpart here.  Single gates from many
// threads are coalesced into batches by a queue per key (Coalescer below).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "params.h"
#include "../../include/tfhe/tfhe.h"
#include "../../include/tfhe_amd.h"
#include "api_internal.h"

using namespace tfhe_amd;
using namespace tfhe_amd::api;

TfheAmdContext *tfhe_amd_context_lane(TfheAmdContext *primary);   // engine.cpp

// ------------------------------------------------------------------ device contexts

static std::atomic<int> g_default_device{0};

static void check(int rc, const char *what) {
    if (rc != TFHE_AMD_OK) {
        fprintf(stderr, "tfhe_amd: %s failed (rc=%d)\n", what, rc);
        die_dramatically("tfhe_amd: GPU engine error");
    }
}

using Tier1Clock = std::chrono::steady_clock;
static double ms_since(Tier1Clock::time_point &t) {   // and restarts t
    const Tier1Clock::time_point now = Tier1Clock::now();
    const double d = std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
    return d;
}

// One pending single-gate call of the coalescing queue (below).
// Its caller sleeps on the request's own condition variable, so that a finished batch wakes only
// its own callers (and a freed lane one new leader) instead of every thread inside a call.
struct Tier1Req {
    int gate;
    LweSample *r;
    const LweSample *a, *b, *c;
    bool taken = false;   // in a running batch (queue lock)

    int rc = TFHE_AMD_OK;
    std::mutex m;             // wake-up of the caller: done (its batch finished) or a call to lead
    std::condition_variable cv;
    bool signaled = false, done = false;
    // a finished batch's callers are woken as a binary tree over wl: the leader wakes wl[0], wl[1],
    // and the caller at wl[i] wakes wl[2i + 2], wl[2i + 3] (log2 depth instead of one by one)
    std::shared_ptr<std::vector<Tier1Req *>> wl;
    int wi = -1;   // the leader, which is not in wl, is the root
    void wake(bool finished) {   // the request may be gone once m is released with done set
        std::lock_guard<std::mutex> lk(m);
        done = done || finished;
        signaled = true;
        cv.notify_one();
    }
    // sleeps until this request is told to lead (false) or its batch has finished (true)
    bool wait_done() {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return signaled; });
        signaled = false;
        return done;
    }
    void wake_children() {   // own call, after its batch: the woken callers may return from here on
        for (int k = 2 * wi + 2; wl && k < 2 * wi + 4 && k < (int)wl->size(); ++k) (*wl)[k]->wake(true);
    }
};

// Coalescing queue of the Tier-1 gates of one key ("per-thread streams or a
// batching queue").  The reference's CPU callers enter single gates from OpenMP teams
// (Cipher.cpp:83-120, cloud.cpp:389-395); one B = 1 launch per call would occupy 2 waves of one
// CU each, and a process has only 4 hardware queues.  Here a call enqueues its gate; a waiting
// thread becomes the leader of the next batch when a queue lane is free and no other leader is
// collecting: it waits until every thread inside a gate call and not already in a running batch
// has enqueued (at most the adaptive window below), takes every pending gate and runs them on
// that lane — one gate kind as a gate batch, several kinds as one mixed launch per 512 gates.
// Two lanes (own stream + scratch each) alternate, so batch k + 1 is staged and launched while
// batch k is still on the GPU or being unstaged: the queue no longer serialises a whole batch's
// host work with the next one — once the two together exceed one ciphertext per CU; below that
// the next leader waits for the running batch and merges its callers' next gates into one launch.
// A lone thread is its own leader at once (B = 1 latency).  Callers sleep on their own request: a
// finished batch's leader does its callers' bookkeeping and wakes exactly them, and a freed lane
// wakes the oldest pending caller to lead (no wake-up of every thread in the call per batch, which
// serialised 64 threads on the queue lock).
// The window adapts to the callers: it starts at the floor below (200 us),
// follows 4x the average wait that ended with every expected thread enqueued (+ 20 us), and
// shrinks by a quarter after a wait that timed out (callers busy elsewhere), within [200, 1000] us.
constexpr int kQueueLanes = 2;
// the straggler window never drops below this: released callers come back within ~0.1 ms, and a
// window that times out on them splits a team into partial batches (which then queue behind each
// other); a caller that does not come back costs one such wait, after which it is no longer expected
constexpr double kWindowFloorUs = 200.0;
namespace {   // this file's own: its steps are not part of the library's surface
struct Coalescer {
    std::mutex mu;
    std::condition_variable arrive_cv;   // a collecting leader waits here for stragglers
    std::vector<Tier1Req *> pending;
    int inside = 0;       // threads inside a Tier-1 gate call on this key
    int in_flight = 0;    // gates taken by running batches
    int running = 0;      // batches running (<= kQueueLanes)
    int returning = 0;    // callers released by finished batches, expected back with their next gate
    bool collecting = false;   // a leader is waiting for stragglers
    bool lane_busy[kQueueLanes] = {false, false};
    int merge_limit = 256;     // gates two lanes' batches may hold together and still merge: one
                               // ciphertext per CU of the key's device (set when the key registers)
    double window_us = kWindowFloorUs;   // adaptive straggler window
    double wait_avg_us = 0.0;
    long long batches = 0, gates = 0, largest = 0, overlapped = 0;
    // where a batch's time goes (ms, summed over batches; tfhe_amd_tier1_queue_times):
    // 0 the leader's straggler wait, 1 packing, 2 the device gate batch (staging, copies, kernels,
    // synchronize), 3 the current_variance sums on the device (mixed kinds; single-kind batches
    // sum them inside 2), 4 unpacking
    double ms[5] = {0, 0, 0, 0, 0};

    // every thread inside a call and not in a running batch has enqueued, and so have the callers
    // the last batch released (an OpenMP team's threads come straight back with their next gate):
    // without them a team of T threads splits into alternating partial batches instead of one of T
    bool expected_all_in() const { return (int)pending.size() >= inside - in_flight + returning; }

    // The steps of one gate call, in order (gate1).  All but await_turn run under mu from start to
    // end; mu may take a request's m inside it (appoint), never the reverse.

    // enter: the call's request joins the pending gates
    void enter(Tier1Req *req) {
        inside += 1;
        if (returning > 0) returning -= 1;
        pending.push_back(req);
        // a collecting leader waits for every expected caller: wake it only when this arrival completes
        // the set (not once per arrival: with 64 callers on a 16-CPU share those wake-ups cost as much
        // as the batch's own host work)
        if (collecting && expected_all_in()) arrive_cv.notify_all();
    }

    // await a turn: true with the queue lock held when the request is to lead the next batch (a free
    // lane and no leader collecting), false without it when another thread's batch has done the request
    bool await_turn(std::unique_lock<std::mutex> &lk, Tier1Req *req) {
        for (;;) {
            if (!req->taken && !collecting && running < kQueueLanes) return true;
            lk.unlock();
            if (req->wait_done()) return false;
            lk.lock();
        }
    }

    // collect: claims a free lane, waits for who is expected and takes every pending gate as the batch
    std::vector<Tier1Req *> collect(std::unique_lock<std::mutex> &lk, int *lane, double *bms) {
        *lane = (int)(std::find(lane_busy, lane_busy + kQueueLanes, false) - lane_busy);
        lane_busy[*lane] = true;
        running += 1;
        collecting = true;
        Tier1Clock::time_point t = Tier1Clock::now();
        // merge instead of overlap: while the other lane's batch runs and both together would still
        // hold at most one ciphertext per CU, a second launch beside it only shares its CUs (two
        // latency-class launches of 31 run 2.15 ms each; one of 62 about 1.8), so wait for that batch
        // and take its callers' next gates too
        if (in_flight > 0 && (int)pending.size() + in_flight <= merge_limit) {
            arrive_cv.wait(lk, [&] { return in_flight == 0; });
            bms[0] += ms_since(t);
        }
        if (!expected_all_in()) {   // the straggler window
            const bool all_in = arrive_cv.wait_for(lk, std::chrono::duration<double, std::micro>(window_us),
                                                   [&] { return expected_all_in(); });
            const double waited_ms = ms_since(t);
            adapt_window(all_in, 1000.0 * waited_ms);
            bms[0] += waited_ms;
        }
        collecting = false;
        std::vector<Tier1Req *> batch;
        batch.swap(pending);
        for (Tier1Req *x : batch) x->taken = true;
        in_flight += (int)batch.size();
        if (running > 1) overlapped += 1;
        return batch;
    }

    void adapt_window(bool all_in, double waited_us) {
        if (all_in) {
            wait_avg_us = wait_avg_us > 0 ? 0.8 * wait_avg_us + 0.2 * waited_us : waited_us;
            window_us = std::min(1000.0, std::max(kWindowFloorUs, 4.0 * wait_avg_us + 20.0));
        } else {
            window_us = std::max(kWindowFloorUs, 0.75 * window_us);
            returning = 0;   // the released callers did not come back: stop expecting them
        }
    }

    // retire: the batch has run; its callers' bookkeeping, done by the leader for all of them
    void retire(const std::vector<Tier1Req *> &batch, int lane, const double *bms) {
        for (int k = 0; k < 5; ++k) ms[k] += bms[k];
        const int n = (int)batch.size();
        in_flight -= n;
        inside -= n;       // every caller of the batch (the leader too) leaves now ...
        returning += n;    // ... and may come back with its next gate
        running -= 1;
        lane_busy[lane] = false;
        batches += 1;
        gates += n;
        largest = std::max(largest, (long long)n);
        arrive_cv.notify_all();   // a collecting leader's expected count changed
        appoint();                // this lane is free again
    }

    // a free lane and no leader collecting: the oldest pending request's thread is asked to lead
    void appoint() {
        if (!collecting && running < kQueueLanes && !pending.empty()) pending.front()->wake(false);
    }
};
}   // namespace

struct KeyEntry {
    uint64_t id;
    const LweKeySwitchKey *ks = nullptr;
    TfheAmdContext *primary = nullptr;
    std::vector<TfheAmdContext *> lanes;
    std::mutex mu;
    Coalescer q;
    TfheAmdContext *qlane[kQueueLanes] = {nullptr, nullptr};   // the queue's lanes (one leader each at a time)
    double *d_var = nullptr;           // KSK row variances [1024][8][4] on the primary's device
};
static std::mutex g_reg_mu;
static std::unordered_map<const void *, std::shared_ptr<KeyEntry>> g_reg;   // bkFFT or KSK -> entry
static std::atomic<uint64_t> g_next_id{1};

static std::shared_ptr<KeyEntry> entry_for(const LweBootstrappingKeyFFT *bkfft, const LweKeySwitchKey *ks) {
    const void *k = bkfft ? (const void *)bkfft : (const void *)ks;
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = g_reg.find(k);
    if (it != g_reg.end()) return it->second;
    if (!bkfft) {   // a KSK that belongs to a registered bkFFT shares its context
        for (auto &kv : g_reg)
            if (kv.second->ks == ks) return kv.second;
    }
    auto e = std::make_shared<KeyEntry>();
    e->id = g_next_id++;
    e->ks = bkfft ? bkfft->ks : ks;
    std::vector<int32_t> flat_ks((size_t)kN * kKsT * kKsBase * (kn + 1));
    ksk_flatten(e->ks, flat_ks.data());
    int rc = tfhe_amd_context_create_raw(bkfft ? bk_coef_of(bkfft) : nullptr, flat_ks.data(), g_default_device.load(),
                                         &e->primary);
    if (rc != TFHE_AMD_OK) {
        fprintf(stderr, "tfhe_amd: cannot create the device context (rc=%d): no usable MI355X/HIP device\n", rc);
        die_dramatically("tfhe_amd: GPU engine unavailable");
    }
    e->q.merge_limit = tfhe_amd_internal_device_cus(tfhe_amd_context_device(e->primary));
    g_reg[k] = e;
    return e;
}

void tfhe_amd::api::forget_device_keys(const void *k1, const void *k2) {
    std::vector<std::shared_ptr<KeyEntry>> dead;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        for (const void *k : {k1, k2}) {
            auto it = g_reg.find(k);
            if (it != g_reg.end()) {
                dead.push_back(it->second);
                g_reg.erase(it);
            }
        }
    }
    for (auto &e : dead) {
        std::lock_guard<std::mutex> lk(e->mu);
        for (auto *l : e->lanes) tfhe_amd_context_destroy(l);
        e->lanes.clear();
        for (auto *&ql : e->qlane) {
            if (ql) tfhe_amd_context_destroy(ql);
            ql = nullptr;
        }
        if (e->d_var) tfhe_amd_internal_free(tfhe_amd_context_device(e->primary), e->d_var);
        e->d_var = nullptr;
        tfhe_amd_context_destroy(e->primary);
        e->primary = nullptr;
    }
}

// This thread's lanes (own stream + scratch) on each key's device.  A thread that exits gives
// its lanes back (the holder's destructor), so callers that spawn short-lived threads (a
// std::thread per request, non-pooled OpenMP teams) do not accumulate streams, scratch and
// pinned memory per thread; a key deleted first has already destroyed its lanes (the weak
// reference is then expired, or the lane is no longer listed).
struct LaneHolder {
    struct Slot {
        std::weak_ptr<KeyEntry> entry;
        TfheAmdContext *lane;
    };
    std::unordered_map<uint64_t, Slot> slots;
    ~LaneHolder() {
        for (auto &kv : slots) {
            std::shared_ptr<KeyEntry> e = kv.second.entry.lock();
            if (!e) continue;
            std::lock_guard<std::mutex> lk(e->mu);
            auto it = std::find(e->lanes.begin(), e->lanes.end(), kv.second.lane);
            if (it == e->lanes.end()) continue;
            e->lanes.erase(it);
            tfhe_amd_context_destroy(kv.second.lane);
        }
    }
};

static TfheAmdContext *lane_for(const LweBootstrappingKeyFFT *bkfft, const LweKeySwitchKey *ks) {
    thread_local LaneHolder holder;
    std::shared_ptr<KeyEntry> e = entry_for(bkfft, ks);
    auto it = holder.slots.find(e->id);
    if (it != holder.slots.end()) return it->second.lane;
    std::lock_guard<std::mutex> lk(e->mu);
    TfheAmdContext *l = tfhe_amd_context_lane(e->primary);
    if (!l) die_dramatically("tfhe_amd: cannot create a per-thread GPU lane");
    e->lanes.push_back(l);
    holder.slots[e->id] = LaneHolder::Slot{e, l};
    return l;
}

// the entry of a key that has one (the statistics below do not create device contexts)
static std::shared_ptr<KeyEntry> find_entry(const TFheGateBootstrappingCloudKeySet *bk) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = g_reg.find(bk->bkFFT);
    return it == g_reg.end() ? nullptr : it->second;
}

// the queue's lane li (own stream + scratch), made on first use; null on failure
static TfheAmdContext *queue_lane(KeyEntry &e, int li) {
    std::lock_guard<std::mutex> lk(e.mu);
    if (!e.qlane[li]) e.qlane[li] = tfhe_amd_context_lane(e.primary);
    return e.qlane[li];
}

// lanes currently alive for the Tier-1 key of `bk` (tests: threads give their lanes back)
EXPORT int tfhe_amd_tier1_lane_count(const TFheGateBootstrappingCloudKeySet *bk) {
    if (!bk || !bk->bkFFT) return TFHE_AMD_E_ARG;
    std::shared_ptr<KeyEntry> e = find_entry(bk);
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return (int)e->lanes.size();
}

EXPORT int tfhe_amd_set_default_device(int device) {
    if (device < 0) return TFHE_AMD_E_ARG;
    g_default_device = device;
    return TFHE_AMD_OK;
}

EXPORT int tfhe_amd_context_create(const TFheGateBootstrappingCloudKeySet *bk, int device, TfheAmdContext **out) {
    if (!bk || !bk->bkFFT || !out) return TFHE_AMD_E_ARG;
    std::vector<int32_t> flat_ks((size_t)kN * kKsT * kKsBase * (kn + 1));
    ksk_flatten(bk->bkFFT->ks, flat_ks.data());
    return tfhe_amd_context_create_raw(bk_coef_of(bk->bkFFT), flat_ks.data(), device, out);
}


// ------------------------------------------------------------------ bootstrapping API

// current_variance of a key-switched sample, as the reference computes it: lweKeySwitch
// (lwe-keyswitch-functions.cu:955-987) starts from lweNoiselessTrivial (variance 0) and every
// lweSubTo of a key-switching-key row (lweKeySwitchTranslate_fromArray :101-127) adds that row's
// variance (lwe-functions.cu:150), in the same i, j order (so the double sum is the same).
// Bookkeeping only: excluded from the Torus32 parity.
static double ks_variance(const LweKeySwitchKey *ks, const int32_t *u_a) {
    const uint32_t prec = 1u << (32 - (1 + ks->basebit * ks->t));
    const uint32_t mask = (uint32_t)ks->base - 1;
    double v = 0.;
    for (int i = 0; i < ks->n; ++i) {
        const uint32_t aibar = (uint32_t)u_a[i] + prec;
        for (int j = 0; j < ks->t; ++j) {
            const uint32_t aij = (aibar >> (32 - (j + 1) * ks->basebit)) & mask;
            if (aij) v += ks->ks[i][j][aij].current_variance;
        }
    }
    return v;
}

// of a lane's last B = 1 gate batch, from its key-switch input (halves = 2 for MUX: u1 + u2)
static double ks_variance_of_last(TfheAmdContext *l, int halves, const LweKeySwitchKey *ks) {
    std::vector<int32_t> u((size_t)halves * kN);
    check(tfhe_amd_internal_last_extracted(l, 1, halves, u.data()), "variance bookkeeping");
    if (halves == 2)
        for (int j = 0; j < kN; ++j) u[j] = (int32_t)((uint32_t)u[j] + (uint32_t)u[kN + j]);
    return ks_variance(ks, u.data());
}

EXPORT void tfhe_bootstrap_woKS_FFT(LweSample *result, const LweBootstrappingKeyFFT *bk, Torus32 mu,
                                    const LweSample *x) {
    TfheAmdContext *l = lane_for(bk, nullptr);
    check(tfhe_amd_bootstrap_woks_batch_host(l, 1, mu, x->a, &x->b, result->a, &result->b), "tfhe_bootstrap_woKS_FFT");
    // the reference's extraction (lwe.cu:41-56, 227-237) leaves current_variance as it was
}

EXPORT void tfhe_bootstrap_FFT(LweSample *result, const LweBootstrappingKeyFFT *bk, Torus32 mu, const LweSample *x) {
    TfheAmdContext *l = lane_for(bk, nullptr);
    check(tfhe_amd_bootstrap_batch_host(l, 1, mu, x->a, &x->b, result->a, &result->b), "tfhe_bootstrap_FFT");
    result->current_variance = ks_variance_of_last(l, 1, bk->ks);
}

EXPORT void lweKeySwitch(LweSample *result, const LweKeySwitchKey *ks, const LweSample *sample) {
    TfheAmdContext *l = lane_for(nullptr, ks);
    const double v = ks_variance(ks, sample->a);   // before: result may alias sample
    check(tfhe_amd_keyswitch_batch_host(l, 1, sample->a, &sample->b, result->a, &result->b), "lweKeySwitch");
    result->current_variance = v;
}

// ------------------------------------------------------------------ L1: blind rotation parts
// tfhe.h:42-43 (lwe-bootstrapping-functions-fft.cu:676-737, 1408-1456) and tgsw_functions.h:70
// (tgsw-fft-operations.cu:124-264) on the key's GPU context, exact (the NTT kernel's arithmetic):
// a caller that holds bk->bkFFT->bkFFT can drive the loop itself, as the reference allows.


static const LweBootstrappingKeyFFT *l1_key(const TGswSampleFFT *gsw, const TGswParams *params, int *index) {
    const LweBootstrappingKeyFFT *f = gsw ? gsw_key_of(gsw, index) : nullptr;
    if (!f) die_dramatically("tfhe_amd: TGswSampleFFT pointer is not part of a bootstrapping key of this library");
    if (params && (params->tlwe_params->N != kN || params->tlwe_params->k != kK || params->l != kL))
        die_dramatically("tfhe_amd: only the default gate-bootstrapping parameter set is supported");
    return f;
}
static void tlwe_to_flat(const TLweSample *s, int32_t *acc) {
    memcpy(acc, s->a[0].coefsT, sizeof(int32_t) * kN);
    memcpy(acc + kN, s->b->coefsT, sizeof(int32_t) * kN);
}
static void flat_to_tlwe(const int32_t *acc, TLweSample *s) {
    memcpy(s->a[0].coefsT, acc, sizeof(int32_t) * kN);
    memcpy(s->b->coefsT, acc + kN, sizeof(int32_t) * kN);
}

// accum <- gsw (x) accum; current_variance 0 as the reference's tLweFFTClear leaves it
EXPORT void tGswFFTExternMulToTLwe(TLweSample *accum, const TGswSampleFFT *gsw, const TGswParams *params) {
    int i = 0;
    const LweBootstrappingKeyFFT *f = l1_key(gsw, params, &i);
    std::vector<int32_t> acc(2 * kN);
    tlwe_to_flat(accum, acc.data());
    check(tfhe_amd_internal_l1(lane_for(f, nullptr), 0, 1, 0, &i, acc.data()), "tGswFFTExternMulToTLwe");
    flat_to_tlwe(acc.data(), accum);
    accum->current_variance = 0.;
}

// n CMux steps with keys bk[0..n) (bk = an element of a key's array; bara_i == 0 skipped, :705);
// current_variance unchanged (each tfhe_MuxRotate_FFT adds the accumulator's to a zero one)
EXPORT void tfhe_blindRotate_FFT(TLweSample *accum, const TGswSampleFFT *bk, const int *bara, const int n,
                                 const TGswParams *bk_params) {
    int i0 = 0;
    const LweBootstrappingKeyFFT *f = l1_key(bk, bk_params, &i0);
    if (n < 0 || i0 + n > kn) die_dramatically("tfhe_blindRotate_FFT: n keys past the end of the key");
    if (n == 0) return;
    std::vector<int32_t> acc(2 * kN), a(kn, 0);
    tlwe_to_flat(accum, acc.data());
    // keys i0 .. i0 + n - 1: steps before i0 are identity (a = 0)
    for (int i = 0; i < n; ++i) a[i0 + i] = (int32_t)(((bara[i] % k2N) + k2N) % k2N);
    check(tfhe_amd_internal_l1(lane_for(f, nullptr), 1, 1, i0 + n, a.data(), acc.data()),
          "tfhe_blindRotate_FFT");
    flat_to_tlwe(acc.data(), accum);
}

// ACC = (0, X^{2N - barb} v) (v itself for barb = 0), blind rotation, extraction at index 0
// (lwe.cu:41-56): result has dimension N; its current_variance is left as it was (lwe.cu)
EXPORT void tfhe_blindRotateAndExtract_FFT(LweSample *result, const TorusPolynomial *v, const TGswSampleFFT *bk,
                                           const int barb, const int *bara, const int n,
                                           const TGswParams *bk_params) {
    int i0 = 0;
    const LweBootstrappingKeyFFT *f = l1_key(bk, bk_params, &i0);
    if (n < 0 || i0 + n > kn) die_dramatically("tfhe_blindRotateAndExtract_FFT: n keys past the end of the key");
    std::vector<int32_t> acc(2 * kN, 0), a(kn, 0);
    const int e = ((k2N - barb) % k2N + k2N) % k2N;   // torusPolynomialMulByXai(2N - barb)
    for (int j = 0; j < kN; ++j) {                   // acc_b[j] = (X^e v)[j]
        int src = j - e;
        uint32_t sign = 0;
        while (src < 0) { src += kN; sign ^= 1; }
        const uint32_t x = (uint32_t)v->coefsT[src];
        acc[kN + j] = (int32_t)(sign ? 0u - x : x);
    }
    if (n > 0) {
        for (int i = 0; i < n; ++i) a[i0 + i] = (int32_t)(((bara[i] % k2N) + k2N) % k2N);
        check(tfhe_amd_internal_l1(lane_for(f, nullptr), 1, 1, i0 + n, a.data(), acc.data()),
              "tfhe_blindRotateAndExtract_FFT");
    }
    result->a[0] = acc[0];
    for (int j = 1; j < kN; ++j) result->a[j] = (int32_t)(0u - (uint32_t)acc[kN - j]);
    result->b = acc[kN];
}

// ------------------------------------------------------------------ gates

// TFHE_AMD_TIER1_COALESCE=0: every thread runs its own B = 1 batches on its own lane (no queue)
static bool coalesce_enabled() {
    static const bool on = [] {
        const char *e = getenv("TFHE_AMD_TIER1_COALESCE");
        return !(e && e[0] == '0');
    }();
    return on;
}

static double *ks_variance_table(const TFheGateBootstrappingCloudKeySet *bk) {
    // the KSK row variances on the device, once per key: each slice's current_variance is summed by
    // k_ks_variance (the reference's order of double adds) instead of on the host from the slice's
    // 4 KB-per-gate key-switch inputs (B = 1024: ~16 ms of host work and a 4 MB copy)
    std::shared_ptr<KeyEntry> e = entry_for(bk->bkFFT, nullptr);
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->d_var) {
        const LweKeySwitchKey *ks = bk->bkFFT->ks;
        std::vector<double> var(kKsVarWords, 0.0);
        bool uniform = true;
        const double v0 = ks->ks[0][0][1].current_variance;
        for (int i = 0; i < kN; ++i)
            for (int j = 0; j < kKsT; ++j)
                for (int h = 0; h < kKsBase; ++h) {
                    const double v = ks->ks[i][j][h].current_variance;
                    var[((size_t)i * kKsT + j) * kKsBase + h] = v;
                    if (h && memcmp(&v, &v0, sizeof v) != 0) uniform = false;   // rows a digit selects
                }
        if (uniform) {   // the sums of k equal terms, added one at a time as the reference does
            var[kKsVarUniform] = 1.0;
            double acc = 0.0;
            for (int k = 0; k <= kN * kKsT; ++k) {
                var[kKsVarUniform + 1 + k] = acc;
                acc += v0;
            }
        }
        void *dv = nullptr;
        if (tfhe_amd_internal_upload(e->primary, var.data(), sizeof(double) * var.size(), &dv)) return nullptr;
        e->d_var = (double *)dv;
    }
    return e->d_var;
}

// an LweSample array as the engine's records
static TfheAmdRows lwe_rows(const LweSample *x) {
    return TfheAmdRows{reinterpret_cast<char *>(const_cast<LweSample *>(x)), sizeof(LweSample), offsetof(LweSample, a),
                       offsetof(LweSample, b), offsetof(LweSample, current_variance)};
}

// A batch of queued gates holding more than one gate kind runs as ONE mixed launch per 512 gates
// (tfhe_amd_gate_batch_mixed_host: one blind rotation + one key switch for all kinds; run_tier1_batch
// below takes the single-kind batches).  Inputs are staged before anything is written, so a result
// may alias any input of its own call; current_variance comes from the device
// (tfhe_amd_internal_mixed_variance, in the reference's order of adds).
static void run_tier1_mixed(TfheAmdContext *l, const std::vector<Tier1Req *> &batch, double *ms,
                            const double *d_var) {
    Tier1Clock::time_point t = Tier1Clock::now();
    std::vector<int32_t> buf;
    std::vector<int> gates;
    std::vector<double> var;
    const int total = (int)batch.size();
    for (int s0 = 0; s0 < total; s0 += 512) {
        const int n = std::min(512, total - s0);
        const size_t A = (size_t)n * kn;
        buf.resize(4 * A + 4 * (size_t)n);   // every word the launch reads is written below
        int32_t *aa = buf.data(), *ba = aa + A, *ca = ba + A, *ra = ca + A;
        int32_t *ab = ra + A, *bb = ab + n, *cb = bb + n, *rb = cb + n;
        gates.resize(n);
        for (int i = 0; i < n; ++i) {
            const Tier1Req *q = batch[s0 + i];
            gates[i] = q->gate;
            memcpy(aa + (size_t)i * kn, q->a->a, kn * 4); ab[i] = q->a->b;
            memcpy(ba + (size_t)i * kn, q->b->a, kn * 4); bb[i] = q->b->b;
            if (q->gate == TFHE_GATE_MUX) { memcpy(ca + (size_t)i * kn, q->c->a, kn * 4); cb[i] = q->c->b; }
        }
        ms[1] += ms_since(t);
        int rc = tfhe_amd_gate_batch_mixed_host(l, n, gates.data(), ra, rb, aa, ab, ba, bb, ca, cb);
        ms[2] += ms_since(t);
        // current_variance on the device from the launch's own key-switch table (a MUX's u1 + u2)
        var.resize(n);
        if (rc == TFHE_AMD_OK) rc = tfhe_amd_internal_mixed_variance(l, n, d_var, var.data());
        ms[3] += ms_since(t);
        if (rc != TFHE_AMD_OK) {
            for (int i = s0; i < total; ++i) batch[i]->rc = rc;
            return;
        }
        for (int i = 0; i < n; ++i) {
            Tier1Req *q = batch[s0 + i];
            memcpy(q->r->a, ra + (size_t)i * kn, kn * 4);
            q->r->b = rb[i];
            q->r->current_variance = var[i];
        }
        ms[4] += ms_since(t);
    }
}

// One gate kind: the engine's record path (tfhe_amd_internal_gate_batch_rows) gathers each request's
// input rows straight into the lane's pinned staging, scatters the results straight into the callers'
// result samples and sums current_variance on the device, so the batch has no intermediate SoA copies,
// no readback of the key-switch inputs and no per-caller variance sums.
static void run_tier1_batch(TfheAmdContext *l, const std::vector<Tier1Req *> &batch, double *ms,
                            const double *d_var) {
    for (const Tier1Req *q : batch)
        if (q->gate != batch[0]->gate) {
            run_tier1_mixed(l, batch, ms, d_var);
            return;
        }
    Tier1Clock::time_point t = Tier1Clock::now();
    const int gate = batch[0]->gate, n = (int)batch.size();
    const bool mux = gate == TFHE_GATE_MUX;
    // shallow copies of the samples: the a pointers and b values (taken before anything is written,
    // so a result may alias an input of its own call)
    std::vector<LweSample> rec((size_t)4 * n);
    LweSample *ra = rec.data(), *rb = ra + n, *rc3 = rb + n, *rr = rc3 + n;
    for (int i = 0; i < n; ++i) {
        const Tier1Req *q = batch[i];
        ra[i].a = q->a->a; ra[i].b = q->a->b;
        rb[i].a = q->b->a; rb[i].b = q->b->b;
        if (mux) { rc3[i].a = q->c->a; rc3[i].b = q->c->b; }
        rr[i].a = q->r->a;
    }
    const TfheAmdRows res = lwe_rows(rr), in[3] = {lwe_rows(ra), lwe_rows(rb), lwe_rows(rc3)};
    ms[1] += ms_since(t);
    const int rc = tfhe_amd_internal_gate_batch_rows(l, gate, n, &res, in, mux ? 3 : 2, d_var);
    ms[2] += ms_since(t);
    for (int i = 0; i < n; ++i) {
        Tier1Req *q = batch[i];
        q->rc = rc;
        if (rc != TFHE_AMD_OK) continue;
        q->r->b = rr[i].b;
        q->r->current_variance = rr[i].current_variance;
    }
    ms[4] += ms_since(t);
}

// The leader's part of a gate call: one batch of everything pending, on one of the queue's own lanes
// (not the leader thread's: a thread that only ever enqueues needs no lane, and leaders change from
// batch to batch).  Returns with the batch's other callers listed in lead->wl as a binary tree.
static void lead_batch(KeyEntry &e, std::unique_lock<std::mutex> &lk, Tier1Req *lead,
                       const TFheGateBootstrappingCloudKeySet *bk) {
    int li = 0;
    double bms[5] = {0, 0, 0, 0, 0};
    const std::vector<Tier1Req *> batch = e.q.collect(lk, &li, bms);
    lk.unlock();
    TfheAmdContext *l = queue_lane(e, li);
    if (!l) die_dramatically("tfhe_amd: cannot create the Tier-1 queue's GPU lane");
    const double *d_var = ks_variance_table(bk);
    if (!d_var) die_dramatically("tfhe_amd: cannot upload the key-switching key's row variances");
    run_tier1_batch(l, batch, bms, d_var);
    lk.lock();
    e.q.retire(batch, li, bms);
    lk.unlock();
    lead->wl = std::make_shared<std::vector<Tier1Req *>>();
    for (Tier1Req *x : batch)
        if (x != lead) {
            x->wl = lead->wl;
            x->wi = (int)lead->wl->size();
            lead->wl->push_back(x);
        }
}

// TFHE_AMD_TIER1_COALESCE=0: the calling thread's own B = 1 batch on its own lane
static void gate1_uncoalesced(int gate, LweSample *r, const LweSample *a, const LweSample *b, const LweSample *c,
                              const TFheGateBootstrappingCloudKeySet *bk) {
    TfheAmdContext *l = lane_for(bk->bkFFT, nullptr);
    check(tfhe_amd_gate_batch_host(l, gate, 1, r->a, &r->b, a->a, &a->b, b->a, &b->b, c ? c->a : nullptr,
                                   c ? &c->b : nullptr),
          "gate");
    // every gate ends in lweKeySwitch (boot-gates.cu:98-448)
    r->current_variance = ks_variance_of_last(l, gate == TFHE_GATE_MUX ? 2 : 1, bk->bkFFT->ks);
}

static void gate1(int gate, LweSample *r, const LweSample *a, const LweSample *b, const LweSample *c,
                  const TFheGateBootstrappingCloudKeySet *bk) {
    if (!coalesce_enabled()) return gate1_uncoalesced(gate, r, a, b, c, bk);
    std::shared_ptr<KeyEntry> e = entry_for(bk->bkFFT, nullptr);
    Tier1Req req{gate, r, a, b, c};
    std::unique_lock<std::mutex> lk(e->q.mu);
    e->q.enter(&req);
    if (e->q.await_turn(lk, &req)) lead_batch(*e, lk, &req, bk);
    // the batch is done and its bookkeeping with it: the leader (the root, index -1) and every
    // caller it wakes pass the wake-up on to the children 2i + 2 and 2i + 3 of their own index
    req.wake_children();
    check(req.rc, "gate");   // result and current_variance were written by the batch
}

// Builds the key's Tier-1 device context (key upload + conversion, HIP initialisation, the
// queue's lane) now, so that the first gate call pays only its own latency.
EXPORT int tfhe_amd_tier1_prepare(const TFheGateBootstrappingCloudKeySet *bk) {
    if (!bk || !bk->bkFFT) return TFHE_AMD_E_ARG;
    std::shared_ptr<KeyEntry> e = entry_for(bk->bkFFT, nullptr);
    int made = 0;
    for (int li = 0; li < kQueueLanes; ++li) made += queue_lane(*e, li) != nullptr;
    return made == kQueueLanes ? TFHE_AMD_OK : TFHE_AMD_E_HIP;
}

EXPORT int tfhe_amd_tier1_queue_stats(const TFheGateBootstrappingCloudKeySet *bk, long long *batches,
                                      long long *gates, long long *largest, int reset) {
    if (!bk || !bk->bkFFT) return TFHE_AMD_E_ARG;
    long long b = 0, g = 0, m = 0;
    if (std::shared_ptr<KeyEntry> e = find_entry(bk)) {
        std::lock_guard<std::mutex> lk(e->q.mu);
        b = e->q.batches; g = e->q.gates; m = e->q.largest;
        if (reset) e->q.batches = e->q.gates = e->q.largest = 0;
    }
    if (batches) *batches = b;
    if (gates) *gates = g;
    if (largest) *largest = m;
    return TFHE_AMD_OK;
}

EXPORT int tfhe_amd_tier1_queue_times(const TFheGateBootstrappingCloudKeySet *bk, double *ms, int reset) {
    if (!bk || !bk->bkFFT) return TFHE_AMD_E_ARG;
    double m[6] = {0, 0, 0, 0, 0, 0};   // m[5] stays 0: the callers no longer sum current_variance themselves
    if (std::shared_ptr<KeyEntry> e = find_entry(bk)) {
        std::lock_guard<std::mutex> lk(e->q.mu);
        for (int k = 0; k < 5; ++k) {
            m[k] = e->q.ms[k];
            if (reset) e->q.ms[k] = 0;
        }
    }
    if (ms)
        for (int k = 0; k < 6; ++k) ms[k] = m[k];
    return TFHE_AMD_OK;
}

EXPORT void bootsNAND(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_NAND, r, a, b, nullptr, bk); }
EXPORT void bootsOR(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_OR, r, a, b, nullptr, bk); }
EXPORT void bootsAND(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_AND, r, a, b, nullptr, bk); }
EXPORT void bootsXOR(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_XOR, r, a, b, nullptr, bk); }
EXPORT void bootsXNOR(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_XNOR, r, a, b, nullptr, bk); }
EXPORT void bootsNOR(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_NOR, r, a, b, nullptr, bk); }
EXPORT void bootsANDNY(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_ANDNY, r, a, b, nullptr, bk); }
EXPORT void bootsANDYN(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_ANDYN, r, a, b, nullptr, bk); }
EXPORT void bootsORNY(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_ORNY, r, a, b, nullptr, bk); }
EXPORT void bootsORYN(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { gate1(TFHE_GATE_ORYN, r, a, b, nullptr, bk); }
EXPORT void bootsMUX(LweSample *r, const LweSample *a, const LweSample *b, const LweSample *c,
                     const TFheGateBootstrappingCloudKeySet *bk) {
    gate1(TFHE_GATE_MUX, r, a, b, c, bk);
}

// linear gates stay on the host (boot-gates.cu:242-267)
EXPORT void bootsNOT(LweSample *r, const LweSample *a, const TFheGateBootstrappingCloudKeySet *bk) {
    lweNegate(r, a, bk->params->in_out_params);
}
EXPORT void bootsCOPY(LweSample *r, const LweSample *a, const TFheGateBootstrappingCloudKeySet *bk) {
    lweCopy(r, a, bk->params->in_out_params);
}
EXPORT void bootsCONSTANT(LweSample *r, int value, const TFheGateBootstrappingCloudKeySet *bk) {
    const Torus32 MU = modSwitchToTorus32(1, 8);
    lweNoiselessTrivial(r, value ? MU : -MU, bk->params->in_out_params);
}


int tfhe_amd_internal_tier1_batch(const TFheGateBootstrappingCloudKeySet *bk, int gate, int B, int32_t *res_a,
                                  int32_t *res_b, const int32_t *a_a, const int32_t *a_b, const int32_t *b_a,
                                  const int32_t *b_b, const int32_t *c_a, const int32_t *c_b) {
    if (!bk || !bk->bkFFT) return TFHE_AMD_E_ARG;
    TfheAmdContext *l = lane_for(bk->bkFFT, nullptr);
    return tfhe_amd_gate_batch_host(l, gate, B, res_a, res_b, a_a, a_b, b_a, b_b, c_a, c_b);
}

// batched convenience over LweSample arrays: the engine gathers the records' rows straight into
// its pinned staging buffer and scatters the results back, pipelined in slices of one round, with
// current_variance computed on the device (tfhe_amd_internal_gate_batch_rows).  result may be the
// same array as an input.

EXPORT int tfhe_amd_boots_batch(int gate, LweSample *result, const LweSample *a, const LweSample *b,
                                const LweSample *c, int B, const TFheGateBootstrappingCloudKeySet *bk) {
    if (!bk || !bk->bkFFT || B < 0 || !result || !a || !b) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (gate == TFHE_GATE_MUX && !c) return TFHE_AMD_E_ARG;
    if (gate != TFHE_GATE_MUX) c = nullptr;
    TfheAmdContext *l = lane_for(bk->bkFFT, nullptr);
    const double *d_var = ks_variance_table(bk);
    if (!d_var) return TFHE_AMD_E_HIP;
    const TfheAmdRows res = lwe_rows(result), in[3] = {lwe_rows(a), lwe_rows(b), lwe_rows(c ? c : a)};
    return tfhe_amd_internal_gate_batch_rows(l, gate, B, &res, in, c ? 3 : 2, d_var);
}
