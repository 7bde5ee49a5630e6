// context.h — the device context and the frame of its entry points, shared by engine.cpp (device
// entry points) and host_batch.cpp (host-pointer entry points).  Internal, not part of the C ABI:
// what the two files share across their boundary is hidden from the library's symbol table.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "engine.h"
#include "../../include/tfhe_amd.h"

#define TFHE_AMD_HIDDEN __attribute__((visibility("hidden")))

TFHE_AMD_HIDDEN uint64_t next_context_uid();   // never repeats (engine.cpp)

struct TfheAmdContext {
    int device = 0;
    hipStream_t stream = nullptr;
    tfhe_amd::DeviceKey key;
    // scratch (device)
    int cap = 0;
    int32_t *u_a = nullptr;   // [2 cap][kN]   extracted samples (2 halves for MUX)
    int32_t *u_b = nullptr;   // [2 cap]
    int32_t *io = nullptr;    // host-API staging: inputs 3 x (cap x 501) + outputs cap x 501
    uint32_t *gflags = nullptr;   // exactness guard flags: 2 words per ciphertext (2 cap ciphertexts)
    uint32_t *gstats = nullptr;   // guard counters (engine.h Guard), zeroed at creation
    // pinned host staging for the host API
    int32_t *h_io = nullptr;
    void *h_u = nullptr;        // pinned readback of extracted samples (Tier-1 variance bookkeeping)
    size_t h_u_bytes = 0;
    // profiling
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> br_ev, ks_ev;
    double br_ms = 0, ks_ms = 0;
    int br_n = 0, ks_n = 0;
    // host-side state of the context (scratch, staging, trace string, events): every entry point
    // holds it; recursive because the host paths call the device entry points
    std::recursive_mutex mu;
    uint64_t uid = next_context_uid();   // never reused (circuit device states are keyed by it)
    bool shared_key = false;   // lane: the key belongs to another context
    tfhe_amd::StreamFence fence;   // u_a / u_b reuse across caller streams
    // sliced host batches (host_batch.cpp): the copy stream and the events
    hipStream_t copy_in = nullptr;
    hipEvent_t ev_in = nullptr, ev_out[2] = {nullptr, nullptr};
    double *d_vout = nullptr, *h_vout = nullptr;   // record batches: current_variance per result
    int vcap = 0;
    std::string last_kernels;   // kernels of the last batch entry point (tfhe_amd_last_kernels)
    void *mtab = nullptr;       // mixed-gate batches: device row / key-switch tables
    size_t mtab_bytes = 0;
    int mtab_rows = 0;          // rows of the last mixed-gate batch (its key-switch table follows them)
    int32_t *fa_tab = nullptr;  // full-adder tables [2 enc_sum + enc_carry][kN] (tfhe_amd_full_add_batch_*), made at first use
};

#define HIPCHK(x)                                                                 \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "tfhe_amd: %s failed: %s (%s:%d)\n", #x,              \
                    hipGetErrorString(e_), __FILE__, __LINE__);                   \
            return TFHE_AMD_E_HIP;                                                \
        }                                                                         \
    } while (0)

// Collects the launches of one C-ABI batch call into its context's last_kernels; nested calls
// (the host path calls the device path) keep the outermost scope's sink.  c = null opens nothing:
// the last batch's trace stays as it is.
struct TFHE_AMD_HIDDEN TraceScope {
    std::string *prev;
    explicit TraceScope(TfheAmdContext *c);
    ~TraceScope();
};

struct ProfScope {
    TfheAmdContext *c;
    hipStream_t s;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> *vec;
    hipEvent_t a = nullptr;
    ProfScope(TfheAmdContext *c_, hipStream_t s_, bool br) : c(c_), s(s_), vec(br ? &c_->br_ev : &c_->ks_ev) {
        if (c->prof) {
            (void)hipEventCreate(&a);
            (void)hipEventRecord(a, s);
        }
    }
    ~ProfScope() {
        if (c->prof && a) {
            hipEvent_t b;
            (void)hipEventCreate(&b);
            (void)hipEventRecord(b, s);
            vec->push_back({a, b});
        }
    }
};

// The frame of an entry point: the context's lock, its device current, the launch trace open — the
// order every entry point relies on — then the scratch reserved for `slots` ciphertexts.  rc is
// TFHE_AMD_OK or the frame's failure, to be tested before anything else is done.  trace = false is
// for the read-backs of the last batch's scratch, which leave that batch's trace standing.
struct TFHE_AMD_HIDDEN EntryFrame {
    std::lock_guard<std::recursive_mutex> lock;
    tfhe_amd::DeviceScope dev;
    TraceScope trace;
    int rc;
    EntryFrame(TfheAmdContext *c, int slots, bool open_trace = true)
        : lock(c->mu), dev(c->device), trace(open_trace ? c : nullptr), rc(device_rc()) {
        if (!rc) rc = tfhe_amd_reserve(c, slots);
    }

private:
    int device_rc() const {
        HIPCHK(dev.rc);
        return TFHE_AMD_OK;
    }
};

static inline size_t io_words(int cap) { return (size_t)4 * cap * (tfhe_amd::kn + 1); }

static const int32_t kMu = 1 << 29;   // modSwitchToTorus32(1, 8)

// the exactness guard is always on: there is no switch that turns it off (tfhe_amd_set_guard_threshold
// can only make it stricter)
static inline tfhe_amd::Guard ctx_guard(TfheAmdContext *c) {
    return c->gflags && c->gstats ? tfhe_amd::Guard{c->gflags, c->gstats} : tfhe_amd::Guard{};
}

// a binary gate's prologue (0, c) + sa X + sb Y; false for any other gate, TFHE_GATE_MUX included
TFHE_AMD_HIDDEN bool gate_spec(int gate, int32_t *c, int32_t *sa, int32_t *sb);

// argument ranges the device and the host forms of an entry point check alike
static inline bool many_args_ok(int log_nu, int n_out) {
    return log_nu >= 0 && log_nu <= 4 && n_out >= 1 && n_out <= (1 << log_nu);
}
static inline bool enc_ok(int e) { return e == TFHE_AMD_ENC_GATE || e == TFHE_AMD_ENC_HALF; }
static inline bool full_add_args_ok(TfheAmdContext *c, int B, int enc_sum, int enc_carry, const int32_t *c_a,
                                    const int32_t *c_b) {
    return c && B >= 0 && enc_ok(enc_sum) && enc_ok(enc_carry) && (c_a != nullptr) == (c_b != nullptr);
}
