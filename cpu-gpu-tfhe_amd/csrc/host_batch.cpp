// host_batch.cpp — the host-pointer forms of the Tier-2 (batched) C ABI: everything that exists only
// because a caller's ciphertexts are in host memory.  The copy pool and the pinned-buffer registry,
// the four gate host paths (unsliced, sliced, records, caller-pinned), the mixed-gate batch, the
// staged bootstrap / LUT / full-adder forms and the variance read-backs.  Each stages through the
// context's pinned h_io and device io scratch and calls the device entry points of engine.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "context.h"
#include "api_internal.h"

using namespace tfhe_amd;

// Host staging copies of the host-pointer paths, split over a few persistent threads: one thread
// moves ~10 GB/s, so staging a 1 024-gate batch's 4 MB of inputs and 2 MB of results took 0.17 ms
// of the call's 0.3 ms copy overhead and a 4 096-gate batch's 1 ms (scripts/host_copy_ubench.cpp,
// profiles/r04b_host_copy_ubench.jsonl: 4 threads 0.05 / 0.19 ms).  Copies below 1 MB in all, and
// calls that find the pool busy (another context copying), run on the caller's thread.
// The pool has 3 helper threads.
struct CopyJob {
    void *dst;
    const void *src;
    size_t bytes;
};
class HostCopyPool {
public:
    static HostCopyPool &get() {
        static HostCopyPool *p = new HostCopyPool();   // never destroyed: helpers idle on their cv at exit
        return *p;
    }
    void copy(const CopyJob *jobs, int n) {
        size_t total = 0;
        for (int i = 0; i < n; ++i) total += jobs[i].bytes;
        std::unique_lock<std::mutex> busy(run_mu_, std::try_to_lock);
        if (helpers_ == 0 || total < (1u << 20) || !busy.owns_lock()) {
            for (int i = 0; i < n; ++i) memcpy(jobs[i].dst, jobs[i].src, jobs[i].bytes);
            return;
        }
        // one immutable chunk list per job, shared with the helpers that join it (a helper still
        // finishing an earlier job holds that job's list, never this one's)
        auto job = std::make_shared<Job>();
        constexpr size_t kChunk = 256 * 1024;
        for (int i = 0; i < n; ++i)
            for (size_t o = 0; o < jobs[i].bytes; o += kChunk)
                job->chunks.push_back(CopyJob{(char *)jobs[i].dst + o, (const char *)jobs[i].src + o,
                                              std::min(kChunk, jobs[i].bytes - o)});
        job->left.store((int)job->chunks.size());
        {
            std::lock_guard<std::mutex> lk(mu_);
            cur_ = job;
            ++gen_;
        }
        cv_.notify_all();
        work(*job);
        std::unique_lock<std::mutex> lk(job->mu);
        job->done.wait(lk, [&] { return job->left.load() == 0; });
    }

private:
    struct Job {
        std::vector<CopyJob> chunks;
        std::atomic<int> next{0}, left{0};
        std::mutex mu;
        std::condition_variable done;
    };
    HostCopyPool() {
        helpers_ = 3;
        for (int i = 0; i < helpers_; ++i) std::thread([this] { loop(); }).detach();
    }
    static void work(Job &j) {
        for (;;) {
            const int i = j.next.fetch_add(1);
            if (i >= (int)j.chunks.size()) return;
            memcpy(j.chunks[i].dst, j.chunks[i].src, j.chunks[i].bytes);
            if (j.left.fetch_sub(1) == 1) {
                std::lock_guard<std::mutex> lk(j.mu);
                j.done.notify_all();
            }
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            std::shared_ptr<Job> job;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                job = cur_;
            }
            if (job) work(*job);
        }
    }
    int helpers_ = 0;
    std::mutex run_mu_;                 // one copy job at a time
    std::mutex mu_;
    std::condition_variable cv_;
    uint64_t gen_ = 0;
    std::shared_ptr<Job> cur_;
};
static void host_copy(std::initializer_list<CopyJob> jobs) {
    HostCopyPool::get().copy(jobs.begin(), (int)jobs.size());
}

// TFHE_AMD_HOST_TRACE=1: one stderr line per host-pointer batch call with its host-side phases
// (ms): staging copies, waits for the device, unstaging copies, the whole call
struct HostTrace {
    static bool on() {
        static const bool v = [] {
            const char *e = getenv("TFHE_AMD_HOST_TRACE");
            return e && e[0] == '1';
        }();
        return v;
    }
    using clk = std::chrono::steady_clock;
    clk::time_point t0 = clk::now(), t = t0;
    double stage = 0, wait = 0, unstage = 0, issue = 0;
    void lap(double &acc) {
        if (!on()) return;
        const clk::time_point n = clk::now();
        acc += std::chrono::duration<double, std::milli>(n - t).count();
        t = n;
    }
    void report(const char *what, int B) {
        if (!on()) return;
        fprintf(stderr, "host_trace %s B=%d stage=%.3f issue=%.3f wait=%.3f unstage=%.3f total=%.3f\n", what, B,
                stage, issue, wait, unstage, std::chrono::duration<double, std::milli>(clk::now() - t0).count());
    }
};

// host-pointer batches above one slice are pipelined slice by slice (one unsliced batch, every
// copy in first and every copy out last, measured slower: profiles/r04o_*)
static int host_slice() { return 1024; }

// ------------------------------------------------------------------ shared helpers

// the copy stream of the sliced batches and its events, made at the first batch that needs them
static int ensure_copy_stream(TfheAmdContext *c) {
    if (c->copy_in) return TFHE_AMD_OK;
    HIPCHK(hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking));
    for (hipEvent_t *e : {&c->ev_in, &c->ev_out[0], &c->ev_out[1]})
        HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return TFHE_AMD_OK;
}

// Waits until nothing of this context is in flight.  Copies of earlier slices may still be running
// on the copy stream, which is not ordered against the next call's staging on c->stream: a host
// path that has used the copy stream drains before it returns, on success and on failure alike.
static hipError_t drain(TfheAmdContext *c) {
    const hipError_t e = c->copy_in ? hipStreamSynchronize(c->copy_in) : hipSuccess;
    const hipError_t f = hipStreamSynchronize(c->stream);
    return e != hipSuccess ? e : f;
}

// the variance buffers (device and pinned host) for B results
static int ensure_vout(TfheAmdContext *c, int B) {
    if (B <= c->vcap) return TFHE_AMD_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->h_vout) (void)hipHostFree(c->h_vout);
    if (c->d_vout) (void)hipFree(c->d_vout);
    c->h_vout = nullptr;
    c->d_vout = nullptr;
    c->vcap = 0;
    HIPCHK(hipMalloc(&c->d_vout, sizeof(double) * (size_t)c->cap));
    HIPCHK(hipHostMalloc(&c->h_vout, sizeof(double) * (size_t)c->cap, hipHostMallocDefault));
    c->vcap = c->cap;
    return TFHE_AMD_OK;
}

// the inputs a gate takes: 3 for TFHE_GATE_MUX, 2 for the binary gates, 0 for anything else
static int gate_inputs(int gate) {
    int32_t k0, k1, k2;
    return gate == TFHE_GATE_MUX ? 3 : gate_spec(gate, &k0, &k1, &k2) ? 2 : 0;
}

// ------------------------------------------------------------------ the slice pipeline

// Host batches are pipelined in slices of one blind-rotation round: slice s is computed on the
// context's stream while the copy stream moves slice s + 1 in, and the host stages slice s + 1 and
// unstages slice s - 1 meanwhile.  Slices touch disjoint rows, so a result that aliases an input
// (the same array) is still read before it is written.
//
// Staging layout (pinned h_io and device io alike): slice s's inputs as ONE contiguous block
// at word 501 nin s0 — [a_0 | a_1 (| a_2) | b_0 | b_1 (| b_2)] — and its results at
// 3 * 501 B + 501 s0 — [res_a | res_b].  One copy per slice and direction: the input block is
// large enough for the copy engine (SDMA), which runs beside the blind rotation of the
// previous slice; the small per-array copies of the round-2 layout went to blit kernels that
// could not start while a blind rotation held every CU (rocprofv3 trace: 3.1-3.4 ms stalls),
// serialising the pipeline.  The result copy is a blit kernel too, so it is issued on the
// compute stream right behind its key switch, ahead of the next slice's blind rotation.  A batch
// of one slice copies in on the compute stream itself (no cross-stream event on the latency path).
//
// stage_in(s0, n, hi) fills the input block hi of slice [s0, s0 + n) from the caller's memory and
// stage_out(s0, n, ho) empties its result block ho into it.  d_var (the KSK row variances on the
// device, or null): each slice's current_variance comes from k_ks_variance on the slice's extracted
// samples, queued right behind its key switch and copied out with its results into c->h_vout.
// Whatever fails — a HIP call, the device batch, an unstage — the pipeline drains before it returns.
template <class StageIn, class StageOut>
static int slice_pipeline(TfheAmdContext *c, int gate, int B, int nin, StageIn stage_in, StageOut stage_out,
                          const double *d_var, const char *label) {
    int rc = ensure_copy_stream(c);
    if (!rc && d_var) rc = ensure_vout(c, B);
    if (rc) return rc;
    constexpr size_t R = kn + 1;
    int32_t *h = c->h_io, *d = c->io;
    const size_t out0 = 3 * R * (size_t)B;
    const int S = host_slice();
    const int nsl = (B + S - 1) / S;
    HostTrace tr;
    auto issue = [&](int s) -> int {
        const int s0 = s * S, n = std::min(S, B - s0);
        const size_t na = (size_t)n * kn, blk = R * (size_t)nin * s0;
        int32_t *hi = h + blk, *di = d + blk;
        tr.lap(tr.issue);
        stage_in(s0, n, hi);
        tr.lap(tr.stage);
        HIPCHK(hipMemcpyAsync(di, hi, R * (size_t)nin * n * 4, hipMemcpyHostToDevice, nsl > 1 ? c->copy_in : c->stream));
        if (nsl > 1) {
            HIPCHK(hipEventRecord(c->ev_in, c->copy_in));
            HIPCHK(hipStreamWaitEvent(c->stream, c->ev_in, 0));
        }
        const int32_t *da = di, *db = di + nin * na;
        int32_t *dout = d + out0 + R * (size_t)s0;
        const int r = tfhe_amd_gate_batch_dev(c, gate, n, dout, dout + na, da, db, da + na, db + n,
                                              nin > 2 ? da + 2 * na : nullptr, nin > 2 ? db + 2 * n : nullptr,
                                              c->stream);
        if (r) return r;
        if (d_var) HIPCHK(launch_ks_variance(c->u_a, n, nin > 2 ? 2 : 1, d_var, c->d_vout + s0, c->stream));
        HIPCHK(hipMemcpyAsync(h + out0 + R * (size_t)s0, dout, R * (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        if (d_var)
            HIPCHK(hipMemcpyAsync(c->h_vout + s0, c->d_vout + s0, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(c->ev_out[s & 1], c->stream));
        return TFHE_AMD_OK;
    };
    auto unstage = [&](int s) -> int {
        const int s0 = s * S, n = std::min(S, B - s0);
        tr.lap(tr.issue);
        HIPCHK(hipEventSynchronize(c->ev_out[s & 1]));
        tr.lap(tr.wait);
        stage_out(s0, n, h + out0 + R * (size_t)s0);
        tr.lap(tr.unstage);
        return TFHE_AMD_OK;
    };
    for (int s = 0; s <= nsl && !rc; ++s) {   // slice s goes out, then slice s - 1 comes home
        if (s < nsl) rc = issue(s);
        if (!rc && s > 0) rc = unstage(s - 1);
    }
    if (rc) {
        (void)drain(c);
        return rc;
    }
    tr.report(label, B);
    return TFHE_AMD_OK;
}

// the array form (tfhe_amd_gate_batch_host above one slice): a and b arrays through the copy pool
static int gate_batch_host_sliced(TfheAmdContext *c, int gate, int B, int32_t *res_a, int32_t *res_b,
                                  const int32_t *const in_a[3], const int32_t *const in_b[3], int nin) {
    auto stage_in = [&](int s0, int n, int32_t *hi) {
        const size_t na = (size_t)n * kn;
        std::vector<CopyJob> jobs;
        for (int k = 0; k < nin; ++k) {
            jobs.push_back({hi + k * na, in_a[k] + (size_t)s0 * kn, na * 4});
            jobs.push_back({hi + nin * na + (size_t)k * n, in_b[k] + s0, (size_t)n * 4});
        }
        HostCopyPool::get().copy(jobs.data(), (int)jobs.size());
    };
    auto stage_out = [&](int s0, int n, const int32_t *ho) {
        host_copy({{res_a + (size_t)s0 * kn, ho, (size_t)n * kn * 4}, {res_b + s0, ho + (size_t)n * kn, (size_t)n * 4}});
    };
    return slice_pipeline(c, gate, B, nin, stage_in, stage_out, nullptr, "sliced");
}

// Record batches (tier1.cpp tfhe_amd_boots_batch over LweSample arrays).  The records' rows
// are gathered by the copy pool straight into the pinned staging buffer (no intermediate SoA copy)
// and the results scattered back the same way, with each result's current_variance.
static inline int32_t *rec_a(const TfheAmdRows &r, int i) {
    return *reinterpret_cast<int32_t *const *>(r.base + (size_t)i * r.stride + r.a_off);
}
static inline int32_t &rec_b(const TfheAmdRows &r, int i) {
    return *reinterpret_cast<int32_t *>(r.base + (size_t)i * r.stride + r.b_off);
}
static inline double &rec_v(const TfheAmdRows &r, int i) {
    return *reinterpret_cast<double *>(r.base + (size_t)i * r.stride + r.v_off);
}

int tfhe_amd_internal_gate_batch_rows(TfheAmdContext *c, int gate, int B, const TfheAmdRows *res,
                                      const TfheAmdRows *in, int nin, const double *d_var) {
    if (!c || B < 0 || !res || !in || nin < 2 || nin > 3 || !d_var) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (gate_inputs(gate) != nin) return TFHE_AMD_E_ARG;
    if (!c->key.has_bk || !c->key.ksk) return TFHE_AMD_E_ARG;
    EntryFrame f(c, B);
    if (f.rc) return f.rc;
    std::vector<CopyJob> jobs;
    auto gather = [&](int s0, int n, int32_t *hi) {
        const size_t na = (size_t)n * kn;
        jobs.clear();
        for (int k = 0; k < nin; ++k)
            for (int i = 0; i < n; ++i) jobs.push_back({hi + k * na + (size_t)i * kn, rec_a(in[k], s0 + i), (size_t)kn * 4});
        HostCopyPool::get().copy(jobs.data(), (int)jobs.size());
        for (int k = 0; k < nin; ++k)
            for (int i = 0; i < n; ++i) hi[nin * na + (size_t)k * n + i] = rec_b(in[k], s0 + i);
    };
    auto scatter = [&](int s0, int n, const int32_t *ho) {
        jobs.clear();
        for (int i = 0; i < n; ++i) jobs.push_back({rec_a(*res, s0 + i), ho + (size_t)i * kn, (size_t)kn * 4});
        HostCopyPool::get().copy(jobs.data(), (int)jobs.size());
        const int32_t *hb = ho + (size_t)n * kn;
        for (int i = 0; i < n; ++i) {
            rec_b(*res, s0 + i) = hb[i];
            rec_v(*res, s0 + i) = c->h_vout[s0 + i];
        }
    };
    return slice_pipeline(c, gate, B, nin, gather, scatter, d_var, "records");
}

// ------------------------------------------------------------------ caller-owned pinned buffers

// Caller-owned pinned buffers.  A registry of the library's own page-locked
// allocations, [start, start + bytes): a call whose every array lies inside one of them DMAs straight
// from and to the caller's memory.  Caching hipHostRegister of arbitrary caller arrays was ruled out
// (a registration outlives a free + malloc that reuses the address); here the library
// allocates and frees, so a registered range is always the memory it was registered for.
namespace {
class PinnedRegistry {
public:
    static PinnedRegistry &get() {
        static PinnedRegistry *r = new PinnedRegistry();   // never destroyed: used from atexit paths
        return *r;
    }
    void add(void *p, size_t bytes) {
        std::lock_guard<std::mutex> lk(mu_);
        blocks_[(uintptr_t)p] = bytes;
    }
    bool remove(void *p) {
        std::lock_guard<std::mutex> lk(mu_);
        return blocks_.erase((uintptr_t)p) != 0;
    }
    bool contains(const void *p, size_t bytes) {
        if (!p) return false;
        const uintptr_t a = (uintptr_t)p;
        std::lock_guard<std::mutex> lk(mu_);
        auto it = blocks_.upper_bound(a);
        if (it == blocks_.begin()) return false;
        --it;
        return a >= it->first && bytes <= it->second && a - it->first <= it->second - bytes;
    }

private:
    std::mutex mu_;
    std::map<uintptr_t, size_t> blocks_;
};
}  // namespace

extern "C" void *tfhe_amd_host_alloc(size_t bytes) {
    if (bytes == 0) bytes = 1;
    void *p = nullptr;
    // mapped into every device's address space at the same address: the pinned path's kernels read
    // the caller's inputs through these pointers (zero-copy over PCIe), so that is checked, not assumed
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess || !p) {
        (void)hipGetLastError();
        return nullptr;
    }
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess || dp != p) {
        (void)hipGetLastError();
        (void)hipHostFree(p);
        return nullptr;
    }
    PinnedRegistry::get().add(p, bytes);
    return p;
}

extern "C" int tfhe_amd_host_free(void *p) {
    if (!p || !PinnedRegistry::get().remove(p)) return TFHE_AMD_E_ARG;
    return hipHostFree(p) == hipSuccess ? TFHE_AMD_OK : TFHE_AMD_E_HIP;
}

extern "C" int tfhe_amd_host_is_pinned(const void *p, size_t bytes) {
    return PinnedRegistry::get().contains(p, bytes) ? 1 : 0;
}

// A host batch whose arrays are all caller-owned pinned buffers: no staging and no input copy.
// Page-locked host memory is mapped into every GPU's address space, so the blind rotation's gate
// prologue (and the guard's exact recomputation) read each ciphertext's inputs straight from the
// caller's arrays over PCIe — 4 KB per ciphertext, all workgroups at once — instead of a copy in
// before the launch (r05c trace, B = 1 024: two 2 MB H2D DMAs of 41.7 us each plus two blit copies
// of the b words and the gaps between them, ~120 us before the blind rotation could start).  The
// results go the other way by DMA (the key switch writes them to device memory first: its split-K
// form adds with atomics, which are not for PCIe-mapped memory): per slice of one round, the slice's
// result copy runs on the copy stream behind its key switch while the next slice's blind rotation
// runs.  (Copying the inputs in by DMA first measured slower: 1.064x against 1.043x the device
// call at B = 1 024, profiles/r05d_*.)  Slices touch disjoint rows, so results that alias inputs are
// still read before they are written.
static int gate_batch_host_pinned(TfheAmdContext *c, int gate, int B, int32_t *res_a, int32_t *res_b,
                                  const int32_t *const in_a[3], const int32_t *const in_b[3], int nin) {
    constexpr size_t R = kn + 1;
    const int S = host_slice();
    const int nsl = (B + S - 1) / S;
    if (nsl > 1) {
        const int rc = ensure_copy_stream(c);
        if (rc) return rc;
    }
    int32_t *d = c->io;
    const size_t out0 = 3 * R * (size_t)B;
    HostTrace tr;
    hipError_t e = hipSuccess;
    for (int s = 0; s < nsl && e == hipSuccess; ++s) {
        const int s0 = s * S, n = std::min(S, B - s0);
        const size_t na = (size_t)n * kn;
        const int32_t *xa[3], *xb[3];
        for (int k = 0; k < nin; ++k) {
            xa[k] = in_a[k] + (size_t)s0 * kn;
            xb[k] = in_b[k] + s0;
        }
        int32_t *dout = d + out0 + R * (size_t)s0;
        const int rc = tfhe_amd_gate_batch_dev(c, gate, n, dout, dout + na, xa[0], xb[0], xa[1], xb[1],
                                               nin > 2 ? xa[2] : nullptr, nin > 2 ? xb[2] : nullptr, c->stream);
        if (rc) {
            (void)drain(c);
            return rc;
        }
        hipStream_t cout = c->stream;
        if (nsl > 1) {   // the result copy beside the next slice's blind rotation
            e = hipEventRecord(c->ev_out[s & 1], c->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(c->copy_in, c->ev_out[s & 1], 0);
            cout = c->copy_in;
        }
        if (e == hipSuccess) e = hipMemcpyAsync(res_a + (size_t)s0 * kn, dout, na * 4, hipMemcpyDeviceToHost, cout);
        if (e == hipSuccess) e = hipMemcpyAsync(res_b + s0, dout + na, (size_t)n * 4, hipMemcpyDeviceToHost, cout);
    }
    tr.lap(tr.issue);
    // the call's wait for its results; after a failed slice, the drain every host path owes
    const hipError_t w = drain(c);
    tr.lap(tr.wait);
    HIPCHK(e);
    HIPCHK(w);
    tr.report("pinned", B);
    return TFHE_AMD_OK;
}

// host batch: stage inputs into pinned memory, one H2D, the device batch, one D2H (sliced and
// pipelined above one round); arrays that are all caller-owned pinned buffers skip the staging.
extern "C" int tfhe_amd_gate_batch_host(TfheAmdContext *c, int gate, int B, int32_t *res_a, int32_t *res_b,
                                        const int32_t *ca_a, const int32_t *ca_b, const int32_t *cb_a,
                                        const int32_t *cb_b, const int32_t *cc_a, const int32_t *cc_b) {
    if (!c || B < 0) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!res_a || !res_b || !ca_a || !ca_b || !cb_a || !cb_b) return TFHE_AMD_E_ARG;
    const int nin = gate_inputs(gate);   // refuse an unknown gate before anything is staged or enqueued
    if (!nin || (nin > 2 && (!cc_a || !cc_b))) return TFHE_AMD_E_ARG;
    if (!c->key.has_bk || !c->key.ksk) return TFHE_AMD_E_ARG;
    EntryFrame f(c, B);
    if (f.rc) return f.rc;
    const int32_t *in_a[3] = {ca_a, cb_a, cc_a}, *in_b[3] = {ca_b, cb_b, cc_b};
    {
        PinnedRegistry &pr = PinnedRegistry::get();
        const size_t A = (size_t)B * kn * 4, Bb = (size_t)B * 4;
        bool pinned = pr.contains(res_a, A) && pr.contains(res_b, Bb);
        for (int k = 0; k < nin && pinned; ++k) pinned = pr.contains(in_a[k], A) && pr.contains(in_b[k], Bb);
        if (pinned) return gate_batch_host_pinned(c, gate, B, res_a, res_b, in_a, in_b, nin);
    }
    if (B > host_slice()) return gate_batch_host_sliced(c, gate, B, res_a, res_b, in_a, in_b, nin);
    const size_t A = (size_t)B * kn;
    // staging layout: the inputs contiguous, [ca_a | cb_a | (cc_a) | ca_b | cb_b | (cc_b)], and
    // the results [res_a | res_b] at 3 (A + B): one copy in and one copy out per call (a
    // single-gate Tier-1 call is latency-bound; each small copy is a few microseconds)
    int32_t *h = c->h_io;
    int32_t *d = c->io;
    int32_t *hb = h + nin * A, *db = d + nin * A;
    HostTrace tr;
    {
        // staged and copied in in two row halves above 512 gates (each >= 1 MB, so that the copy
        // pool takes it), the first half's copy in flight while the second is staged: of the copy
        // in, only the second half's stays on the call's critical path
        const int nch = B > 512 ? 2 : 1;
        std::vector<CopyJob> jobs;
        tr.lap(tr.issue);
        for (int ch = 0; ch < nch; ++ch) {
            const size_t r0 = (size_t)B * ch / nch, r1 = (size_t)B * (ch + 1) / nch;
            jobs.clear();
            for (int k = 0; k < nin; ++k) {
                jobs.push_back({h + k * A + r0 * kn, in_a[k] + r0 * kn, (r1 - r0) * kn * 4});
                jobs.push_back({hb + (size_t)k * B + r0, in_b[k] + r0, (r1 - r0) * 4});
            }
            HostCopyPool::get().copy(jobs.data(), (int)jobs.size());
            for (int k = 0; k < nin; ++k)
                HIPCHK(hipMemcpyAsync(d + k * A + r0 * kn, h + k * A + r0 * kn, (r1 - r0) * kn * 4,
                                      hipMemcpyHostToDevice, c->stream));
            if (ch == nch - 1)
                HIPCHK(hipMemcpyAsync(db, hb, (size_t)nin * B * 4, hipMemcpyHostToDevice, c->stream));
        }
        tr.lap(tr.stage);
    }
    int32_t *hr = h + 3 * (A + B), *dr = d + 3 * (A + B);
    const int rc = tfhe_amd_gate_batch_dev(c, gate, B, dr, dr + A, d, db, d + A, db + B,
                                           nin > 2 ? d + 2 * A : nullptr, nin > 2 ? db + 2 * B : nullptr, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(hr, dr, (A + B) * 4, hipMemcpyDeviceToHost, c->stream));
    tr.lap(tr.issue);
    HIPCHK(hipStreamSynchronize(c->stream));
    tr.lap(tr.wait);
    host_copy({{res_a, hr, A * 4}, {res_b, hr + A, (size_t)B * 4}});
    tr.lap(tr.unstage);
    tr.report("unsliced", B);
    return TFHE_AMD_OK;
}

// B gates of mixed kinds (gates[i] = TFHE_GATE_NAND .. TFHE_GATE_MUX) in ONE blind-rotation launch
// and ONE key-switch launch: the batch is a one-level circuit of one instance — wires 3i, 3i + 1,
// 3i + 2 hold gate i's inputs a, b (, c), wire 3B + i its result; gate i contributes one row
// (c, sa, sb) = its prologue (boot-gates.cu:98-397), a MUX two rows and a combined key switch
// (:407-448), in request order (row r of the extracted samples: gate i's first row, then its
// second for a MUX).  The rows kernel is the circuit path's k_blind_rotate_v6_rows, guarded.
// cc_* may be null when no gate is a MUX.  res may alias inputs.
extern "C" int tfhe_amd_gate_batch_mixed_host(TfheAmdContext *c, int B, const int *gates, int32_t *res_a,
                                              int32_t *res_b, const int32_t *ca_a, const int32_t *ca_b,
                                              const int32_t *cb_a, const int32_t *cb_b, const int32_t *cc_a,
                                              const int32_t *cc_b) {
    if (!c || B < 0) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!gates || !res_a || !res_b || !ca_a || !ca_b || !cb_a || !cb_b) return TFHE_AMD_E_ARG;
    if (!c->key.has_bk || !(c->key.ksk4 || c->key.ksk5)) return TFHE_AMD_E_ARG;
    int nmux = 0;
    for (int i = 0; i < B; ++i) {
        const int nin = gate_inputs(gates[i]);
        if (!nin) return TFHE_AMD_E_ARG;
        nmux += nin > 2;
    }
    if (nmux && (!cc_a || !cc_b)) return TFHE_AMD_E_ARG;
    const int rows = B + nmux;
    std::vector<CircRow> rw((size_t)rows);
    std::vector<CircKs> ks((size_t)B);
    for (int i = 0, r = 0; i < B; ++i) {
        if (gates[i] == TFHE_GATE_MUX) {
            rw[r] = CircRow{-kMu, 1, 1, 0, 3 * i, 3 * i + 1, -1, 0};
            rw[r + 1] = CircRow{-kMu, -1, 1, 0, 3 * i, 3 * i + 2, -1, 0};
            ks[i] = CircKs{r, r + 1, kMu, 3 * B + i};
            r += 2;
        } else {
            int32_t k0, k1, k2;
            gate_spec(gates[i], &k0, &k1, &k2);
            rw[r] = CircRow{k0, k1, k2, 0, 3 * i, 3 * i + 1, -1, 0};
            ks[i] = CircKs{r, -1, 0, 3 * B + i};
            r += 1;
        }
    }
    EntryFrame f(c, std::max(B, (rows + 1) / 2));   // u / guard scratch for `rows` rows
    if (f.rc) return f.rc;
    const size_t tab = sizeof(CircRow) * rw.size() + sizeof(CircKs) * ks.size();
    if (tab > c->mtab_bytes) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->mtab) (void)hipFree(c->mtab);
        c->mtab = nullptr;
        c->mtab_bytes = 0;
        HIPCHK(hipMalloc(&c->mtab, tab));
        c->mtab_bytes = tab;
    }
    hipStream_t s = c->stream;
    HIPCHK(c->fence.acquire(s));
    // wires: a [4B][500], b [4B] in the io scratch (4 cap x 501 words), staged the same way on the host
    const size_t WA = (size_t)4 * B * kn;
    int32_t *h = c->h_io, *d = c->io;
    const int32_t *in_a[3] = {ca_a, cb_a, cc_a}, *in_b[3] = {ca_b, cb_b, cc_b};
    for (int i = 0; i < B; ++i)
        for (int k = 0; k < (gates[i] == TFHE_GATE_MUX ? 3 : 2); ++k) {
            memcpy(h + (size_t)(3 * i + k) * kn, in_a[k] + (size_t)i * kn, kn * 4);
            h[WA + 3 * i + k] = in_b[k][i];
        }
    HIPCHK(hipMemcpyAsync(d, h, (size_t)3 * B * kn * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d + WA, h + WA, (size_t)3 * B * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->mtab, rw.data(), sizeof(CircRow) * rw.size(), hipMemcpyHostToDevice, s));
    const CircKs *d_ks = (const CircKs *)((char *)c->mtab + sizeof(CircRow) * rw.size());
    c->mtab_rows = rows;
    HIPCHK(hipMemcpyAsync((void *)d_ks, ks.data(), sizeof(CircKs) * ks.size(), hipMemcpyHostToDevice, s));
    {
        ProfScope ps(c, s, true);
        const Guard gd = ctx_guard(c);
        HIPCHK(launch_blind_rotate_rows(c->key, 1, rows, (const CircRow *)c->mtab, d, d + WA, kMu, c->u_a, c->u_b, s,
                                        BrMode::Const, &gd));
    }
    {
        ProfScope ps(c, s, false);
        HIPCHK(launch_keyswitch_rows(c->key, 1, B, d_ks, c->u_a, c->u_b, d, d + WA, s));
    }
    int32_t *hr = h + (size_t)3 * B * kn;
    HIPCHK(hipMemcpyAsync(hr, d + (size_t)3 * B * kn, (size_t)B * kn * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h + WA + 3 * B, d + WA + 3 * B, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c->fence.done(s));
    HIPCHK(hipStreamSynchronize(s));   // also: the host tables above may be freed on return
    memcpy(res_a, hr, (size_t)B * kn * 4);
    memcpy(res_b, h + WA + 3 * B, (size_t)B * 4);
    return TFHE_AMD_OK;
}

// ------------------------------------------------------------------ staged forms

// Pinned staging of the staged host paths below.  The caller lists its input arrays and its output
// arrays (host pointer, 32-bit words; a null pointer is an absent block of no words); the blocks lie
// back to back, inputs first, at the same offsets in the pinned h_io and the device io.  upload
// stages every input and issues one copy in; after the device call, download issues one copy out,
// waits for it and unstages the outputs.  Every input is staged before anything is written back, so
// outputs may alias inputs.
namespace {
struct HostIn {
    const int32_t *p;
    size_t words;
};
struct HostOut {
    int32_t *p;
    size_t words;
};
class Staging {
public:
    Staging(std::initializer_list<HostIn> in, std::initializer_list<HostOut> out) : in_(in), out_(out) {
        for (HostIn &b : in_) {
            if (!b.p) b.words = 0;
            in_words_ += b.words;
        }
        for (HostOut &b : out_) {
            if (!b.p) b.words = 0;
            out_words_ += b.words;
        }
    }
    // the capacity (tfhe_amd_reserve) whose io scratch holds every block
    size_t cap() const { return (in_words_ + out_words_ + io_words(1) - 1) / io_words(1); }
    // device addresses of input / output block i (null: absent)
    const int32_t *in(const TfheAmdContext *c, size_t i) const {
        size_t off = 0;
        for (size_t k = 0; k < i; ++k) off += in_[k].words;
        return in_[i].p ? c->io + off : nullptr;
    }
    int32_t *out(const TfheAmdContext *c, size_t i) const {
        size_t off = in_words_;
        for (size_t k = 0; k < i; ++k) off += out_[k].words;
        return out_[i].p ? c->io + off : nullptr;
    }
    int upload(TfheAmdContext *c) const {
        size_t off = 0;
        for (const HostIn &b : in_) {
            if (b.words) memcpy(c->h_io + off, b.p, b.words * 4);
            off += b.words;
        }
        HIPCHK(hipMemcpyAsync(c->io, c->h_io, in_words_ * 4, hipMemcpyHostToDevice, c->stream));
        return TFHE_AMD_OK;
    }
    int download(TfheAmdContext *c) const {
        size_t off = in_words_;
        HIPCHK(hipMemcpyAsync(c->h_io + off, c->io + off, out_words_ * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (const HostOut &b : out_) {
            if (b.words) memcpy(b.p, c->h_io + off, b.words * 4);
            off += b.words;
        }
        return TFHE_AMD_OK;
    }

private:
    std::vector<HostIn> in_;
    std::vector<HostOut> out_;
    size_t in_words_ = 0, out_words_ = 0;
};
}  // namespace

// woKS / bootstrap / KS host versions
enum { OP_WOKS, OP_BOOT, OP_KS };
static int single_input_host(TfheAmdContext *c, int op, int B, int32_t mu, const int32_t *in_a,
                             const int32_t *in_b, int32_t *out_a, int32_t *out_b) {
    if (!c || B < 0) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!in_a || !in_b || !out_a || !out_b) return TFHE_AMD_E_ARG;
    const int din = op == OP_KS ? kN : kn, dout = op == OP_WOKS ? kN : kn;
    // [in_a | in_b | out_a | out_b]: B * (din + dout + 2) <= 1526 B words, within B slots' 2004 B
    const Staging st({{in_a, (size_t)B * din}, {in_b, (size_t)B}}, {{out_a, (size_t)B * dout}, {out_b, (size_t)B}});
    EntryFrame f(c, B);
    if (f.rc) return f.rc;
    int rc = st.upload(c);
    if (rc) return rc;
    const int32_t *d_a = st.in(c, 0), *d_b = st.in(c, 1);
    int32_t *oa = st.out(c, 0), *ob = st.out(c, 1);
    if (op == OP_WOKS) rc = tfhe_amd_bootstrap_woks_batch_dev(c, B, mu, d_a, d_b, oa, ob, c->stream);
    else if (op == OP_BOOT) rc = tfhe_amd_bootstrap_batch_dev(c, B, mu, d_a, d_b, oa, ob, c->stream);
    else rc = tfhe_amd_keyswitch_batch_dev(c, B, d_a, d_b, oa, ob, c->stream);
    if (rc) return rc;
    return st.download(c);
}

extern "C" int tfhe_amd_bootstrap_woks_batch_host(TfheAmdContext *c, int B, int32_t mu, const int32_t *x_a,
                                                  const int32_t *x_b, int32_t *u_a, int32_t *u_b) {
    return single_input_host(c, OP_WOKS, B, mu, x_a, x_b, u_a, u_b);
}
extern "C" int tfhe_amd_bootstrap_batch_host(TfheAmdContext *c, int B, int32_t mu, const int32_t *x_a,
                                             const int32_t *x_b, int32_t *res_a, int32_t *res_b) {
    return single_input_host(c, OP_BOOT, B, mu, x_a, x_b, res_a, res_b);
}
extern "C" int tfhe_amd_keyswitch_batch_host(TfheAmdContext *c, int B, const int32_t *u_a, const int32_t *u_b,
                                             int32_t *res_a, int32_t *res_b) {
    return single_input_host(c, OP_KS, B, 0, u_a, u_b, res_a, res_b);
}

// programmable bootstrap, host arrays: the staged path of single_input_host with the tables
// (n_lut x 4 KB) and the table indices uploaded beside the inputs; n_out >= 1: the many-LUT form
// (the callers have checked log_nu and n_out), n_out = 0: the single-table form
static int lut_batch_host(TfheAmdContext *c, bool ks, int B, int n_lut, const int32_t *tv, const int32_t *lut_index,
                          int32_t cst, int32_t sa, const int32_t *x_a, const int32_t *x_b, int32_t sb,
                          const int32_t *y_a, const int32_t *y_b, int32_t *out_a, int32_t *out_b, int log_nu = 0,
                          int n_out = 0) {
    if (!c || B < 0 || n_lut <= 0 || !tv) return TFHE_AMD_E_ARG;
    const size_t n_res = n_out ? n_out : 1;   // outputs per ciphertext, function-major in out
    if (lut_index)
        for (int i = 0; i < B; ++i)
            if (lut_index[i] < 0 || lut_index[i] >= n_lut) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!x_a || !x_b || !out_a || !out_b || (sb && (!y_a || !y_b))) return TFHE_AMD_E_ARG;
    // [x_a | x_b | y_a | y_b | tables | indices | out_a | out_b]
    const size_t Ai = (size_t)B * kn, Bo = n_res * B, Ao = Bo * (ks ? kn : kN);
    const Staging st({{x_a, Ai}, {x_b, (size_t)B}, {sb ? y_a : nullptr, Ai}, {sb ? y_b : nullptr, (size_t)B},
                      {tv, (size_t)n_lut * kN}, {lut_index, (size_t)B}},
                     {{out_a, Ao}, {out_b, Bo}});
    if (st.cap() > ((size_t)1 << 24)) return TFHE_AMD_E_ARG;
    EntryFrame f(c, std::max((int)Bo, (int)st.cap()));
    if (f.rc) return f.rc;
    int rc = st.upload(c);
    if (rc) return rc;
    if (n_out)
        rc = (ks ? tfhe_amd_bootstrap_lut_many_batch_dev : tfhe_amd_bootstrap_lut_many_woks_batch_dev)(
            c, B, n_lut, st.in(c, 4), st.in(c, 5), log_nu, n_out, cst, sa, st.in(c, 0), st.in(c, 1), sb, st.in(c, 2),
            st.in(c, 3), st.out(c, 0), st.out(c, 1), c->stream);
    else
        rc = (ks ? tfhe_amd_bootstrap_lut_batch_dev : tfhe_amd_bootstrap_lut_woks_batch_dev)(
            c, B, n_lut, st.in(c, 4), st.in(c, 5), cst, sa, st.in(c, 0), st.in(c, 1), sb, st.in(c, 2), st.in(c, 3),
            st.out(c, 0), st.out(c, 1), c->stream);
    if (rc) return rc;
    return st.download(c);
}

// the staged path: [a | b | c | res] in the io scratch (5 B x 501 words)
extern "C" int tfhe_amd_full_add_batch_host(TfheAmdContext *c, int B, int enc_sum, int enc_carry, const int32_t *a_a,
                                            const int32_t *a_b, const int32_t *b_a, const int32_t *b_b,
                                            const int32_t *c_a, const int32_t *c_b, int32_t *res_a, int32_t *res_b) {
    if (!full_add_args_ok(c, B, enc_sum, enc_carry, c_a, c_b)) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!a_a || !a_b || !b_a || !b_b || !res_a || !res_b) return TFHE_AMD_E_ARG;
    const size_t Ai = (size_t)B * kn, Bw = (size_t)B;
    const Staging st({{a_a, Ai}, {a_b, Bw}, {b_a, Ai}, {b_b, Bw}, {c_a, Ai}, {c_b, Bw}}, {{res_a, 2 * Ai}, {res_b, 2 * Bw}});
    if (st.cap() > ((size_t)1 << 24)) return TFHE_AMD_E_ARG;
    EntryFrame f(c, std::max(2 * B, (int)st.cap()));   // 2 B: the device form's extracted samples
    if (f.rc) return f.rc;
    int rc = st.upload(c);
    if (rc) return rc;
    rc = tfhe_amd_full_add_batch_dev(c, B, enc_sum, enc_carry, st.in(c, 0), st.in(c, 1), st.in(c, 2), st.in(c, 3),
                                     st.in(c, 4), st.in(c, 5), st.out(c, 0), st.out(c, 1), c->stream);
    if (rc) return rc;
    return st.download(c);
}

extern "C" int tfhe_amd_bootstrap_lut_many_woks_batch_host(TfheAmdContext *c, int B, int n_lut, const int32_t *tv,
                                                           const int32_t *lut_index, int log_nu, int n_out,
                                                           int32_t cst, int32_t sa, const int32_t *x_a,
                                                           const int32_t *x_b, int32_t sb, const int32_t *y_a,
                                                           const int32_t *y_b, int32_t *u_a, int32_t *u_b) {
    if (!many_args_ok(log_nu, n_out)) return TFHE_AMD_E_ARG;
    return lut_batch_host(c, false, B, n_lut, tv, lut_index, cst, sa, x_a, x_b, sb, y_a, y_b, u_a, u_b, log_nu, n_out);
}
extern "C" int tfhe_amd_bootstrap_lut_many_batch_host(TfheAmdContext *c, int B, int n_lut, const int32_t *tv,
                                                      const int32_t *lut_index, int log_nu, int n_out, int32_t cst,
                                                      int32_t sa, const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                                      const int32_t *y_a, const int32_t *y_b, int32_t *res_a,
                                                      int32_t *res_b) {
    if (!many_args_ok(log_nu, n_out)) return TFHE_AMD_E_ARG;
    return lut_batch_host(c, true, B, n_lut, tv, lut_index, cst, sa, x_a, x_b, sb, y_a, y_b, res_a, res_b, log_nu,
                          n_out);
}

extern "C" int tfhe_amd_bootstrap_lut_woks_batch_host(TfheAmdContext *c, int B, int n_lut, const int32_t *tv,
                                                      const int32_t *lut_index, int32_t cst, int32_t sa,
                                                      const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                                      const int32_t *y_a, const int32_t *y_b, int32_t *u_a,
                                                      int32_t *u_b) {
    return lut_batch_host(c, false, B, n_lut, tv, lut_index, cst, sa, x_a, x_b, sb, y_a, y_b, u_a, u_b);
}
extern "C" int tfhe_amd_bootstrap_lut_batch_host(TfheAmdContext *c, int B, int n_lut, const int32_t *tv,
                                                 const int32_t *lut_index, int32_t cst, int32_t sa,
                                                 const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                                 const int32_t *y_a, const int32_t *y_b, int32_t *res_a,
                                                 int32_t *res_b) {
    return lut_batch_host(c, true, B, n_lut, tv, lut_index, cst, sa, x_a, x_b, sb, y_a, y_b, res_a, res_b);
}

// ------------------------------------------------------------------ read-backs of the last batch

// largest batch the host path runs unsliced, i.e. whose key-switch inputs are all in the scratch
// afterwards (tier1.cpp's variance bookkeeping rounds)
int tfhe_amd_internal_unsliced_max() { return host_slice(); }

// The extracted samples (key-switch inputs) of this context's last gate batch of at most one
// round (unsliced host path), halves x B rows of kN words: the Tier-1 API's per-thread-lane mode
// (TFHE_AMD_TIER1_COALESCE=0) and raw tfhe_bootstrap_FFT derive the key-switched output's
// current_variance from their digits (tier1.cpp ks_variance).
int tfhe_amd_internal_last_extracted(TfheAmdContext *c, int B, int halves, int32_t *u_a) {
    if (!c || B <= 0 || halves < 1 || halves > 2 || (size_t)halves * B > 2 * (size_t)c->cap) return TFHE_AMD_E_ARG;
    EntryFrame f(c, 0, false);
    if (f.rc) return f.rc;
    const size_t bytes = sizeof(int32_t) * (size_t)halves * B * kN;
    // through the context's pinned readback buffer: a D2H straight into the caller's (pageable,
    // often freshly allocated) array costs a fixed ~0.3 ms per call
    if (bytes > c->h_u_bytes) {
        if (c->h_u) (void)hipHostFree(c->h_u);
        c->h_u = nullptr;
        c->h_u_bytes = 0;
        HIPCHK(hipHostMalloc(&c->h_u, bytes, hipHostMallocDefault));
        c->h_u_bytes = bytes;
    }
    HIPCHK(hipMemcpyAsync(c->h_u, c->u_a, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    host_copy({{u_a, c->h_u, bytes}});
    return TFHE_AMD_OK;
}

// current_variance of the context's last gate batch (<= one round: its key-switch inputs are still
// in the scratch), computed on the device (k_ks_variance) into out [B]
int tfhe_amd_internal_ks_variance(TfheAmdContext *c, int B, int halves, const double *d_var, double *out) {
    if (!c || B <= 0 || halves < 1 || halves > 2 || (size_t)halves * B > 2 * (size_t)c->cap || !d_var || !out)
        return TFHE_AMD_E_ARG;
    EntryFrame f(c, 0, false);
    if (f.rc) return f.rc;
    double *d_out = reinterpret_cast<double *>(c->io);   // the batch's staging is done with by now
    HIPCHK(launch_ks_variance(c->u_a, B, halves, d_var, d_out, c->stream));
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return TFHE_AMD_OK;
}

// current_variance of the context's last mixed-gate batch (tfhe_amd_gate_batch_mixed_host: its row and
// key-switch tables and extracted samples are still in the scratch), on the device, into out [B]
int tfhe_amd_internal_mixed_variance(TfheAmdContext *c, int B, const double *d_var, double *out) {
    if (!c || B <= 0 || !d_var || !out || !c->mtab || c->mtab_rows < B) return TFHE_AMD_E_ARG;
    EntryFrame f(c, 0, false);
    if (f.rc) return f.rc;
    const int rc = ensure_vout(c, B);
    if (rc) return rc;
    const CircKs *d_ks = (const CircKs *)((char *)c->mtab + sizeof(CircRow) * (size_t)c->mtab_rows);
    HIPCHK(launch_ks_variance_rows(c->u_a, B, d_ks, d_var, c->d_vout, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_vout, c->d_vout, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(out, c->h_vout, sizeof(double) * (size_t)B);
    return TFHE_AMD_OK;
}
