// tgsw_dfa.cpp — leveled automata of the batched C ABI (include/tfhe_amd.h): a
// deterministic automaton over TGSW-encrypted input bits, one exact CMux per live state and bit.  The
// kernel is k_tgsw_dfa_v4 (blind_rotate_v4.hip), launched once per input bit; this file holds the
// automaton (transitions, live sets, state scratch), the argument checks, the slicing, the host
// staging and the host-only builders.  It reaches a context only through tfhe_amd_internal_frame.
// The weighted runs (tfhe_amd_wfa_*) are the same path with two more arrays: every
// transition adds a plaintext monomial, so the result carries values computed along the path.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "engine.h"
#include "tgsw_internal.h"
#include "../../include/tfhe_amd.h"

using namespace tfhe_amd;

#define HIPCHK(x)                                                                 \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "tfhe_amd: %s failed: %s (%s:%d)\n", #x,              \
                    hipGetErrorString(e_), __FILE__, __LINE__);                   \
            return TFHE_AMD_E_HIP;                                                \
        }                                                                         \
    } while (0)

namespace {
constexpr int kMaxStates = 64, kMaxLen = 1024, kMaxOut = 16;
constexpr int kMaxOutWeighted = 64;   // the weighted runs: one output per bit of a 64-bit result
constexpr size_t kScratchBytes = (size_t)256 << 20;   // both state buffers together
}  // namespace

// The automaton on `device` (-1: host only).  d_tab = next [Q][2], then the live sets R_0 ..
// R_{max_len - 1} one after the other (R_i starts at word 2 Q + off[i]); the host keeps R_max_len too.
// scratch: the two state buffers [Bs][Q][2][kN] the steps alternate between, shared by every run on
// the automaton, so their reuse is ordered across streams like a set's tree scratch.
struct TfheAmdDfa {
    int device = -1;
    int Q = 0, start = 0, max_len = 0;
    std::vector<int32_t> next;
    std::vector<int32_t> live;   // concatenated R_0 .. R_max_len
    std::vector<int> off;        // max_len + 2 entries
    int32_t *d_tab = nullptr;
    std::mutex mu;
    int32_t *scratch = nullptr;
    size_t scratch_words = 0;
    StreamFence fence;
};

namespace {

bool next_ok(int Q, const int32_t *next) {
    for (int k = 0; k < 2 * Q; ++k)
        if (next[k] < 0 || next[k] >= Q) return false;
    return true;
}

struct UploadJob {
    TfheAmdDfa *dfa;
};

int upload_in_frame(const ContextFrame &f, void *arg) {
    TfheAmdDfa *d = static_cast<UploadJob *>(arg)->dfa;
    std::vector<int32_t> tab(d->next);
    tab.insert(tab.end(), d->live.begin(), d->live.begin() + d->off[d->max_len]);
    HIPCHK(hipMalloc(&d->d_tab, sizeof(int32_t) * tab.size()));
    HIPCHK(hipMemcpyAsync(d->d_tab, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, f.stream));
    HIPCHK(hipStreamSynchronize(f.stream));   // tab is a local
    d->device = f.device;
    return TFHE_AMD_OK;
}

struct RunJob {
    TfheAmdTgsw *set;
    TfheAmdDfa *dfa;
    bool ks;
    int B, len, n_fin, fin_rows, n_out;
    const int32_t *sel, *fin, *fin_index;
    int32_t *out_a, *out_b;
    // the weighted forms (tfhe_amd_wfa_run_*): w_val [Q][2], w_pos [len], shared by the queries
    bool weighted = false;
    const int32_t *w_val = nullptr, *w_pos = nullptr;
};

RunJob weighted_job(RunJob j, const int32_t *w_val, const int32_t *w_pos) {
    j.weighted = true;
    j.w_val = w_val;
    j.w_pos = w_pos;
    return j;
}

// shape checks shared by the device and host forms (no pointer is read)
bool run_shape_ok(const RunJob &j) {
    if (!j.set || !j.dfa || j.B < 0 || j.len < 1 || j.len > j.dfa->max_len || j.n_fin < 1) return false;
    if ((j.fin_rows != 1 && j.fin_rows != 2) || j.n_out < 1 || j.n_out > (j.weighted ? kMaxOutWeighted : kMaxOut))
        return false;
    return (long)j.B * j.n_out <= 0x3fffffffL && (long)j.B * j.len <= 0x3fffffffL;
}

// the pointers every run with B > 0 needs (none is read here)
bool run_pointers_ok(const RunJob &j) {
    if (!j.sel || !j.fin || !j.out_a || !j.out_b) return false;
    return !j.weighted || (j.w_val && j.w_pos);
}

int run_in_frame(const ContextFrame &f, void *arg) {
    const RunJob &j = *static_cast<RunJob *>(arg);
    TfheAmdDfa *d = j.dfa;
    hipStream_t s = f.stream;
    if (j.ks && !f.key->ksk) return TFHE_AMD_E_ARG;
    int32_t *u_a = j.ks ? f.u_a : j.out_a, *u_b = j.ks ? f.u_b : j.out_b;
    const size_t state_words = (size_t)d->Q * 2 * kN;   // one query's states in one buffer
    const int slice = (int)(kScratchBytes / (2 * sizeof(int32_t) * state_words));   // >= 256 queries
    const int Bs_max = j.B < slice ? j.B : slice;
    std::unique_lock<std::mutex> lock(d->mu, std::defer_lock);
    int32_t *buf[2] = {nullptr, nullptr};
    if (j.len > 1) {
        lock.lock();
        const size_t need = 2 * state_words * Bs_max;
        if (d->scratch_words < need) {
            HIPCHK(hipDeviceSynchronize());   // the scratch may still be in use on another stream
            if (d->scratch) (void)hipFree(d->scratch);
            d->scratch = nullptr;
            d->scratch_words = 0;
            HIPCHK(hipMalloc(&d->scratch, sizeof(int32_t) * need));
            d->scratch_words = need;
        }
        HIPCHK(d->fence.acquire(s));
        buf[0] = d->scratch;
        buf[1] = d->scratch + state_words * Bs_max;
    }
    TgswDfaStep a;
    a.count = j.set->count;
    a.Q = d->Q;
    a.sel_stride = j.len;
    a.next = d->d_tab;
    a.fin = j.fin;
    a.n_fin = j.n_fin;
    a.fin_rows = j.fin_rows;
    a.n_out = j.n_out;
    a.u_stride = j.B;
    a.w_val = j.weighted ? j.w_val : nullptr;
    for (int q0 = 0; q0 < j.B; q0 += Bs_max) {
        a.B = j.B - q0 < Bs_max ? j.B - q0 : Bs_max;
        a.fin_index = j.fin_index ? j.fin_index + q0 : nullptr;
        a.u_a = u_a + (size_t)q0 * kN;
        a.u_b = u_b + q0;
        // step t reads bit t - 1 and computes the states of R_{t-1} from buffer (t + 1) & 1 into t & 1
        for (int t = j.len; t >= 1; --t) {
            a.sel = j.sel + (size_t)q0 * j.len + (t - 1);
            a.w_pos = j.weighted ? j.w_pos + (t - 1) : nullptr;
            a.live = d->d_tab + 2 * d->Q + d->off[t - 1];
            a.n_live = d->off[t] - d->off[t - 1];
            a.src = buf[(t + 1) & 1];
            a.dst = buf[t & 1];
            HIPCHK(launch_tgsw_dfa_v4(*f.key, j.set->v2, a, t == j.len, t == 1, s));
        }
    }
    if (j.len > 1) HIPCHK(d->fence.done(s));
    if (j.ks)   // ONE key switch over the n_out B extracted samples
        HIPCHK(launch_keyswitch(*f.key, j.n_out * j.B, u_a, u_b, nullptr, nullptr, 0, j.out_a, j.out_b, s));
    return TFHE_AMD_OK;
}

int run_dev(TfheAmdContext *c, const RunJob &job, void *stream) {
    const RunJob &j = job;
    if (!c || !run_shape_ok(j)) return TFHE_AMD_E_ARG;
    const int dev = tfhe_amd_context_device(c);
    if (j.set->device != dev || j.set->count <= 0 || j.dfa->device != dev || !j.dfa->d_tab) return TFHE_AMD_E_ARG;
    if (j.B == 0) return TFHE_AMD_OK;
    if (!run_pointers_ok(j)) return TFHE_AMD_E_ARG;
    RunJob copy = j;
    return tfhe_amd_internal_frame(c, stream, j.ks ? j.B * j.n_out : 0, run_in_frame, &copy);
}

struct HostRunJob {
    TfheAmdContext *c;
    RunJob j;   // host pointers
};

int run_host_in_frame(const ContextFrame &f, void *arg) {
    HostRunJob &h = *static_cast<HostRunJob *>(arg);
    const RunJob &j = h.j;
    hipStream_t s = f.stream;
    const size_t n_sel = (size_t)j.B * j.len, n_finw = (size_t)j.n_fin * j.dfa->Q * j.fin_rows * kN;
    const size_t n_res = (size_t)j.n_out * j.B, row = j.ks ? kn : kN;
    DevBufs bufs;
    int32_t *d_sel, *d_fin, *d_idx = nullptr, *d_a, *d_b, *d_wv = nullptr, *d_wp = nullptr;
    HIPCHK(bufs.get(&d_sel, n_sel));
    HIPCHK(bufs.get(&d_fin, n_finw));
    if (j.fin_index) HIPCHK(bufs.get(&d_idx, (size_t)j.B));
    if (j.weighted) {
        HIPCHK(bufs.get(&d_wv, (size_t)2 * j.dfa->Q));
        HIPCHK(bufs.get(&d_wp, (size_t)j.len));
        HIPCHK(hipMemcpyAsync(d_wv, j.w_val, sizeof(int32_t) * 2 * j.dfa->Q, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_wp, j.w_pos, sizeof(int32_t) * j.len, hipMemcpyHostToDevice, s));
    }
    HIPCHK(bufs.get(&d_a, n_res * row));
    HIPCHK(bufs.get(&d_b, n_res));
    HIPCHK(hipMemcpyAsync(d_sel, j.sel, sizeof(int32_t) * n_sel, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_fin, j.fin, sizeof(int32_t) * n_finw, hipMemcpyHostToDevice, s));
    if (j.fin_index) HIPCHK(hipMemcpyAsync(d_idx, j.fin_index, sizeof(int32_t) * j.B, hipMemcpyHostToDevice, s));
    RunJob dj = j;
    dj.sel = d_sel;
    dj.fin = d_fin;
    dj.fin_index = d_idx;
    dj.w_val = d_wv;
    dj.w_pos = d_wp;
    dj.out_a = d_a;
    dj.out_b = d_b;
    hipError_t sync = hipSuccess;
    const int rc = run_dev(h.c, dj, s);
    if (rc == TFHE_AMD_OK) {
        sync = hipMemcpyAsync(j.out_a, d_a, sizeof(int32_t) * n_res * row, hipMemcpyDeviceToHost, s);
        if (sync == hipSuccess) sync = hipMemcpyAsync(j.out_b, d_b, sizeof(int32_t) * n_res, hipMemcpyDeviceToHost, s);
    }
    const hipError_t e = hipStreamSynchronize(s);   // before the buffers go, whatever happened
    if (rc != TFHE_AMD_OK) return rc;
    HIPCHK(sync);
    HIPCHK(e);
    return TFHE_AMD_OK;
}

int run_host(TfheAmdContext *c, const RunJob &j) {
    if (!c || !run_shape_ok(j)) return TFHE_AMD_E_ARG;
    const int dev = tfhe_amd_context_device(c);
    if (j.set->device != dev || j.set->count <= 0 || j.dfa->device != dev || !j.dfa->d_tab) return TFHE_AMD_E_ARG;
    if (j.B == 0) return TFHE_AMD_OK;
    if (!run_pointers_ok(j)) return TFHE_AMD_E_ARG;
    for (size_t k = 0; k < (size_t)j.B * j.len; ++k)
        if (j.sel[k] < 0 || j.sel[k] >= j.set->count) return TFHE_AMD_E_ARG;
    if (j.weighted)
        for (int i = 0; i < j.len; ++i)
            if (j.w_pos[i] < 0 || j.w_pos[i] >= kN) return TFHE_AMD_E_ARG;
    if (j.fin_index)
        for (int q = 0; q < j.B; ++q)
            if (j.fin_index[q] < 0 || j.fin_index[q] >= j.n_fin) return TFHE_AMD_E_ARG;
    HostRunJob h{c, j};
    // the outer frame holds the context (the lock is recursive) from the uploads to the read-back
    return tfhe_amd_internal_frame(c, nullptr, 0, run_host_in_frame, &h);
}

}  // namespace

extern "C" int tfhe_amd_dfa_create(TfheAmdContext *ctx, int n_states, int start, const int32_t *next, int max_len,
                                   TfheAmdDfa **out) {
    if (out) *out = nullptr;
    if (!out || !next || n_states < 1 || n_states > kMaxStates || start < 0 || start >= n_states || max_len < 1 ||
        max_len > kMaxLen || !next_ok(n_states, next))
        return TFHE_AMD_E_ARG;
    TfheAmdDfa *d = new TfheAmdDfa();
    d->Q = n_states;
    d->start = start;
    d->max_len = max_len;
    d->next.assign(next, next + 2 * n_states);
    // R_0 = {start}, R_{i+1} = next[R_i][0 / 1], each in ascending order
    unsigned long long cur = 1ull << start;
    d->off.push_back(0);
    for (int i = 0; i <= max_len; ++i) {
        unsigned long long nxt = 0;
        for (int s = 0; s < n_states; ++s)
            if (cur >> s & 1) {
                d->live.push_back(s);
                nxt |= 1ull << next[2 * s] | 1ull << next[2 * s + 1];
            }
        d->off.push_back((int)d->live.size());
        cur = nxt;
    }
    if (ctx) {
        UploadJob j{d};
        const int rc = tfhe_amd_internal_frame(ctx, nullptr, 0, upload_in_frame, &j);
        if (rc != TFHE_AMD_OK) {
            if (d->d_tab) {
                DeviceScope dev_scope(tfhe_amd_context_device(ctx));
                (void)hipFree(d->d_tab);
            }
            delete d;
            return rc;
        }
    }
    *out = d;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_dfa_destroy(TfheAmdDfa *dfa) {
    if (!dfa) return TFHE_AMD_OK;
    if (dfa->device >= 0) {
        DeviceScope dev_scope(dfa->device);
        (void)hipDeviceSynchronize();   // launches on caller streams may still read the automaton
        dfa->fence.release();
        if (dfa->scratch) (void)hipFree(dfa->scratch);
        if (dfa->d_tab) (void)hipFree(dfa->d_tab);
    }
    delete dfa;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_dfa_info(const TfheAmdDfa *dfa, int *n_states, int *start, int *max_len, int *device) {
    if (!dfa) return TFHE_AMD_E_ARG;
    if (n_states) *n_states = dfa->Q;
    if (start) *start = dfa->start;
    if (max_len) *max_len = dfa->max_len;
    if (device) *device = dfa->device;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_dfa_live(const TfheAmdDfa *dfa, int step, int32_t *states) {
    if (!dfa || step < 0 || step > dfa->max_len) return TFHE_AMD_E_ARG;
    const int n = dfa->off[step + 1] - dfa->off[step];
    if (states) memcpy(states, dfa->live.data() + dfa->off[step], sizeof(int32_t) * n);
    return n;
}

extern "C" int tfhe_amd_dfa_run_woks_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                                         const int32_t *sel, int n_fin, int fin_rows, const int32_t *fin,
                                         const int32_t *fin_index, int n_out, int32_t *u_a, int32_t *u_b,
                                         void *stream) {
    return run_dev(ctx, RunJob{set, dfa, false, B, len, n_fin, fin_rows, n_out, sel, fin, fin_index, u_a, u_b}, stream);
}

extern "C" int tfhe_amd_dfa_run_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                                    const int32_t *sel, int n_fin, int fin_rows, const int32_t *fin,
                                    const int32_t *fin_index, int n_out, int32_t *res_a, int32_t *res_b,
                                    void *stream) {
    return run_dev(ctx, RunJob{set, dfa, true, B, len, n_fin, fin_rows, n_out, sel, fin, fin_index, res_a, res_b},
                   stream);
}

extern "C" int tfhe_amd_dfa_run_woks_host(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                                          const int32_t *sel, int n_fin, int fin_rows, const int32_t *fin,
                                          const int32_t *fin_index, int n_out, int32_t *u_a, int32_t *u_b) {
    return run_host(ctx, RunJob{set, dfa, false, B, len, n_fin, fin_rows, n_out, sel, fin, fin_index, u_a, u_b});
}

extern "C" int tfhe_amd_dfa_run_host(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                                     const int32_t *sel, int n_fin, int fin_rows, const int32_t *fin,
                                     const int32_t *fin_index, int n_out, int32_t *res_a, int32_t *res_b) {
    return run_host(ctx, RunJob{set, dfa, true, B, len, n_fin, fin_rows, n_out, sel, fin, fin_index, res_a, res_b});
}

// ---- weighted runs: the same path with the transition weights behind sel

extern "C" int tfhe_amd_wfa_run_woks_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                                         const int32_t *sel, const int32_t *w_val, const int32_t *w_pos, int n_fin,
                                         int fin_rows, const int32_t *fin, const int32_t *fin_index, int n_out,
                                         int32_t *u_a, int32_t *u_b, void *stream) {
    return run_dev(ctx, weighted_job(RunJob{set, dfa, false, B, len, n_fin, fin_rows, n_out, sel, fin, fin_index, u_a, u_b},
                                     w_val, w_pos), stream);
}

extern "C" int tfhe_amd_wfa_run_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                                    const int32_t *sel, const int32_t *w_val, const int32_t *w_pos, int n_fin,
                                    int fin_rows, const int32_t *fin, const int32_t *fin_index, int n_out,
                                    int32_t *res_a, int32_t *res_b, void *stream) {
    return run_dev(ctx, weighted_job(RunJob{set, dfa, true, B, len, n_fin, fin_rows, n_out, sel, fin, fin_index, res_a, res_b},
                                     w_val, w_pos), stream);
}

extern "C" int tfhe_amd_wfa_run_woks_host(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                                          const int32_t *sel, const int32_t *w_val, const int32_t *w_pos, int n_fin,
                                          int fin_rows, const int32_t *fin, const int32_t *fin_index, int n_out,
                                          int32_t *u_a, int32_t *u_b) {
    return run_host(ctx, weighted_job(RunJob{set, dfa, false, B, len, n_fin, fin_rows, n_out, sel, fin, fin_index, u_a, u_b},
                                      w_val, w_pos));
}

extern "C" int tfhe_amd_wfa_run_host(TfheAmdContext *ctx, TfheAmdTgsw *set, TfheAmdDfa *dfa, int B, int len,
                                     const int32_t *sel, const int32_t *w_val, const int32_t *w_pos, int n_fin,
                                     int fin_rows, const int32_t *fin, const int32_t *fin_index, int n_out,
                                     int32_t *res_a, int32_t *res_b) {
    return run_host(ctx, weighted_job(RunJob{set, dfa, true, B, len, n_fin, fin_rows, n_out, sel, fin, fin_index, res_a, res_b},
                                      w_val, w_pos));
}

// ---- builders (host only)

extern "C" int tfhe_amd_dfa_build_compare(int32_t *next, int *start, int32_t *cls) {
    if (!next || !start) return TFHE_AMD_E_ARG;
    // 0: x = y so far; 1: x < y and 2: x > y, decided by a more significant pair (absorbing);
    // 3 / 4: x = y so far and this pair's x bit read, 0 / 1
    const int32_t t[5][2] = {{3, 4}, {1, 1}, {2, 2}, {0, 1}, {2, 0}};
    memcpy(next, t, sizeof(t));
    *start = 0;
    if (cls) {
        const int32_t c[5] = {TFHE_AMD_DFA_EQ, TFHE_AMD_DFA_LT, TFHE_AMD_DFA_GT, TFHE_AMD_DFA_MID, TFHE_AMD_DFA_MID};
        memcpy(cls, c, sizeof(c));
    }
    return 5;
}

extern "C" int tfhe_amd_dfa_build_contains(int m, const int32_t *pattern, int32_t *next, int *start) {
    if (!pattern || !next || !start || m < 1 || m > 63) return TFHE_AMD_E_ARG;
    for (int k = 0; k < m; ++k)
        if (pattern[k] != 0 && pattern[k] != 1) return TFHE_AMD_E_ARG;
    // Knuth-Morris-Pratt: x = the state of the pattern without its first bit, i.e. where a mismatch
    // in state k falls back to
    next[0] = next[1] = 0;
    next[pattern[0]] = 1;
    int x = 0;
    for (int k = 1; k < m; ++k) {
        next[2 * k] = next[2 * x];
        next[2 * k + 1] = next[2 * x + 1];
        next[2 * k + pattern[k]] = k + 1;
        x = next[2 * x + pattern[k]];
    }
    next[2 * m] = next[2 * m + 1] = m;
    *start = 0;
    return m + 1;
}

extern "C" int tfhe_amd_dfa_build_at_least(int t, int32_t *next, int *start) {
    if (!next || !start || t < 1 || t > 63) return TFHE_AMD_E_ARG;
    for (int k = 0; k <= t; ++k) {
        next[2 * k] = k;
        next[2 * k + 1] = k < t ? k + 1 : t;
    }
    *start = 0;
    return t + 1;
}

extern "C" int tfhe_amd_dfa_fin_fill(int n_states, int n_out, const int32_t *values, int32_t *fin) {
    if (!values || !fin || n_states < 1 || n_states > kMaxStates || n_out < 1 || n_out > kMaxOut) return TFHE_AMD_E_ARG;
    memset(fin, 0, sizeof(int32_t) * (size_t)n_states * kN);
    for (int s = 0; s < n_states; ++s)
        for (int f = 0; f < n_out; ++f) fin[(size_t)s * kN + f] = values[s * n_out + f];
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_dfa_simulate(int n_states, int start, const int32_t *next, int len, const int32_t *bits) {
    if (!next || n_states < 1 || n_states > kMaxStates || start < 0 || start >= n_states || len < 0 ||
        (len > 0 && !bits) || !next_ok(n_states, next))
        return TFHE_AMD_E_ARG;
    int s = start;
    for (int i = 0; i < len; ++i) {
        if (bits[i] != 0 && bits[i] != 1) return TFHE_AMD_E_ARG;
        s = next[2 * s + bits[i]];
    }
    return s;
}

// ---- weighted builders (host only)

extern "C" int tfhe_amd_wfa_build_max(int d, int want_max, int32_t *next, int *start, int32_t *w_val, int32_t *w_pos) {
    if (!next || !start || !w_val || !w_pos || d < 1 || d > 64) return TFHE_AMD_E_ARG;
    // 0: x = y so far, an x bit comes; 1 / 2: x = y so far and this pair's x bit read, 0 / 1;
    // 3 / 4: x < y decided, an x / a y bit comes; 5 / 6: x > y decided, an x / a y bit comes.
    // The decided states alternate so that the position-independent weights tell the bits apart.
    enum { EQ, MID0, MID1, LTX, LTY, GTX, GTY };
    const int32_t t[7][2] = {{MID0, MID1}, {EQ, LTX}, {GTX, EQ}, {LTY, LTY}, {LTX, LTX}, {GTY, GTY}, {GTX, GTX}};
    memcpy(next, t, sizeof(t));
    *start = EQ;
    const int32_t one = 1 << 30;
    memset(w_val, 0, sizeof(int32_t) * 14);
    // the weight sits on the transition that knows the result's bit: in an undecided pair the y bit's
    // (x = y = 1; x < y gives y = 1 to the maximum, x > y gives x = 1 to it, and 0 to the minimum)
    w_val[2 * MID1 + 1] = one;
    if (want_max) {
        w_val[2 * MID0 + 1] = one;
        w_val[2 * MID1 + 0] = one;
    }
    // decided: x < y takes y's bits for the maximum and x's for the minimum, x > y the other way
    w_val[2 * (want_max ? LTY : LTX) + 1] = one;
    w_val[2 * (want_max ? GTX : GTY) + 1] = one;
    for (int k = 0; k < d; ++k) w_pos[2 * k] = w_pos[2 * k + 1] = d - 1 - k;   // pair k holds bit d - 1 - k
    return 7;
}

extern "C" int tfhe_amd_wfa_build_popcount(int len, int p, int32_t *next, int *start, int32_t *w_val, int32_t *w_pos) {
    if (!next || !start || !w_val || !w_pos || (p != 2 && p != 4 && p != 8 && p != 16) || len < 1 || len > p - 1)
        return TFHE_AMD_E_ARG;
    next[0] = next[1] = 0;
    *start = 0;
    w_val[0] = 0;
    w_val[1] = (int32_t)((1ll << 32) / (2 * p));   // one step of the LUT digit (2 c + 1) / (4 p)
    for (int i = 0; i < len; ++i) w_pos[i] = 0;
    return 1;
}

extern "C" int tfhe_amd_wfa_build_first_one(int len, int32_t *next, int *start, int32_t *w_val, int32_t *w_pos) {
    if (!next || !start || !w_val || !w_pos || len < 1 || len > 64) return TFHE_AMD_E_ARG;
    // 0: no set bit seen; 1: seen (absorbing, weightless)
    const int32_t t[2][2] = {{0, 1}, {1, 1}};
    memcpy(next, t, sizeof(t));
    *start = 0;
    memset(w_val, 0, sizeof(int32_t) * 4);
    w_val[1] = 1 << 30;
    for (int i = 0; i < len; ++i) w_pos[i] = i;
    return 2;
}

extern "C" int tfhe_amd_wfa_fin_fill(int n_states, int n_out, int32_t value, int32_t *fin) {
    if (!fin || n_states < 1 || n_states > kMaxStates || n_out < 1 || n_out > kMaxOutWeighted) return TFHE_AMD_E_ARG;
    memset(fin, 0, sizeof(int32_t) * (size_t)n_states * kN);
    for (int s = 0; s < n_states; ++s)
        for (int f = 0; f < n_out; ++f) fin[(size_t)s * kN + f] = value;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_wfa_simulate(int n_states, int start, const int32_t *next, const int32_t *w_val,
                                     const int32_t *w_pos, int len, const int32_t *bits, int32_t *poly) {
    if (!next || !w_val || !poly || n_states < 1 || n_states > kMaxStates || start < 0 || start >= n_states || len < 0 ||
        (len > 0 && (!bits || !w_pos)) || !next_ok(n_states, next))
        return TFHE_AMD_E_ARG;
    for (int i = 0; i < len; ++i)
        if ((bits[i] != 0 && bits[i] != 1) || w_pos[i] < 0 || w_pos[i] >= kN) return TFHE_AMD_E_ARG;
    memset(poly, 0, sizeof(int32_t) * kN);
    int s = start;
    for (int i = 0; i < len; ++i) {
        poly[w_pos[i]] = (int32_t)((uint32_t)poly[w_pos[i]] + (uint32_t)w_val[2 * s + bits[i]]);
        s = next[2 * s + bits[i]];
    }
    return s;
}
