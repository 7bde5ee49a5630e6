// engine.cpp — device contexts, key upload, scratch and the device forms of the Tier-2 (batched)
// C ABI (the host-pointer forms: host_batch.cpp).
//
// Replaces the reference GPU host glue: key upload (gpuParallel/main.cu:165-213, 236-254,
// 364-407), the per-gate chunking / temp allocation of bootsAND_fullGPU_n_Bit
// (boot-gates.cu:2845-2915) and bootstrapAndKeySwitch_n_Bit (:2481-2629).  Differences
// by design: keys are uploaded once per (cloud key, GPU) in the coefficient domain and
// converted on the device; ciphertext b-halves stay on the device; no per-call FFT plans,
// no host round trips inside a batch; work is enqueued on a caller-chosen stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "context.h"
#include "api_internal.h"
#include "ntt_tables.h"

namespace tfhe_amd {

// ------------------------------------------------------------------ tables

uint32_t host_powmod(uint32_t b, uint64_t e, uint32_t q) {
    uint64_t r = 1, x = b % q;
    while (e) {
        if (e & 1) r = r * x % q;
        x = x * x % q;
        e >>= 1;
    }
    return (uint32_t)r;
}

static unsigned brv(unsigned x, int bits) {
    unsigned r = 0;
    for (int i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}
static uint32_t shoup(uint32_t w, uint32_t q) { return (uint32_t)(((uint64_t)w << 32) / q); }

void build_ntt_tables(NttTables *t) {
    for (int s = 0; s < 2; s++) {
        const uint32_t q = kQ[s];
        uint32_t psi = 0;
        for (uint32_t g = 2; g < 1000 && !psi; g++) {
            const uint32_t c = host_powmod(g, (q - 1) / k2N, q);
            if (host_powmod(c, kN, q) == q - 1) psi = c;   // primitive 2N-th root
        }
        const uint32_t ipsi = host_powmod(psi, q - 2, q);
        for (int k = 0; k < kN; k++) {
            t->psi[s][k] = host_powmod(psi, brv(k, kLogN), q);
            t->psip[s][k] = shoup(t->psi[s][k], q);
            t->ipsi[s][k] = host_powmod(ipsi, brv(k, kLogN), q);
            t->ipsip[s][k] = shoup(t->ipsi[s][k], q);
        }
        t->ninv[s] = host_powmod(kN, q - 2, q);
        // -q^-1 mod 2^32 by Newton iteration
        uint32_t inv = q;
        for (int it = 0; it < 5; it++) inv *= 2u - q * inv;
        t->qinv_neg[s] = 0u - inv;
        const uint32_t r_mod_q = (uint32_t)((1ull << 32) % q);
        t->bk_scale[s] = (uint32_t)((uint64_t)t->ninv[s] * r_mod_q % q);
        t->bk_scalep[s] = shoup(t->bk_scale[s], q);
    }
    t->crt_h = host_powmod(kQ[0] % kQ[1], kQ[1] - 2, kQ[1]);
    t->crt_hp = shoup(t->crt_h, kQ[1]);
}

// the calling thread's trace sink: the context of the batch entry point it is in (TraceScope)
static thread_local std::string *g_trace = nullptr;
void trace_kernel(const char *name) {
    if (!g_trace) return;
    const size_t n = strlen(name);
    for (size_t p = 0; p < g_trace->size();) {   // once per name, in first-launch order
        const size_t e = g_trace->find(',', p);
        const size_t len = (e == std::string::npos ? g_trace->size() : e) - p;
        if (len == n && g_trace->compare(p, n, name) == 0) return;
        if (e == std::string::npos) break;
        p = e + 1;
    }
    if (!g_trace->empty()) g_trace->push_back(',');
    g_trace->append(name);
}

static std::atomic<int> g_br_version{-1};

// The library carries the default fp64 kernel (v6) and the exact NTT kernel (v4: the guard's
// fallback, the L1 entry points and the exact reference generation); the earlier and experimental
// generations (v1 LDS radix-2, v2, v3, v5 latency, v7 shared-key, v8 four-wave) were retired in
// round 4 (their measurements: DESIGN.md, profiles/README.md).
static bool br_available(int v) { return v == 0 || v == 4 || v == 6; }

int br_version() {   // 0 (v6, guarded) until tfhe_amd_select_kernel picks another
    const int v = g_br_version.load(std::memory_order_relaxed);
    return v < 0 ? 0 : v;
}

// high word of the rounding distance at which the exact kernel recomputes a ciphertext: 1/8
// (0x3FC00000) by default — 1.6x the largest distance real keys show (0.06-0.08), so that an
// error can only escape by reaching 7/8 at a coefficient while every other rounding of the
// ciphertext's 500 steps stays below 1/8; tfhe_amd_set_guard_threshold lowers
// it (tests force the fallback with 0) and refuses anything above 1/8
static std::atomic<uint32_t> g_guard_hi{0x3FC00000u};
uint32_t guard_threshold_hi() { return g_guard_hi.load(std::memory_order_relaxed); }

// the default fp64 kernel, then the exact kernel in guard mode over the flags it wrote
static hipError_t run_v6_guarded(const DeviceKey &key, int B, int halves, const BrInput *in, int32_t mu,
                                 int32_t *u_a, int32_t *u_b, hipStream_t s, const Guard *guard) {
    hipError_t e = launch_blind_rotate_v6(key, B, halves, in, mu, u_a, u_b, s, guard);
    if (e != hipSuccess || !guard || !guard->flags) return e;
    return launch_blind_rotate_v4(key, B, halves, in, mu, u_a, u_b, s, guard);
}

static hipError_t run_br(const DeviceKey &key, int B, int halves, const BrInput *in, int32_t mu, int32_t *u_a,
                         int32_t *u_b, hipStream_t s, const Guard *guard) {
    switch (br_version()) {
    case 4: return launch_blind_rotate_v4(key, B, halves, in, mu, u_a, u_b, s);
    default: return run_v6_guarded(key, B, halves, in, mu, u_a, u_b, s, guard);   // 0, 6
    }
}

hipError_t launch_blind_rotate_rows(const DeviceKey &key, int B, int nrows, const CircRow *rows, const int32_t *wa,
                                    const int32_t *wb, int32_t mu, int32_t *u_a, int32_t *u_b, hipStream_t s,
                                    BrMode mode, const Guard *guard) {
    if (br_version() == 4) return launch_blind_rotate_v4_rows(key, B, nrows, rows, wa, wb, mu, u_a, u_b, s, mode);
    hipError_t e = launch_blind_rotate_v6_rows(key, B, nrows, rows, wa, wb, mu, u_a, u_b, s, mode, guard);
    if (e != hipSuccess || !guard || !guard->flags) return e;
    return launch_blind_rotate_v4_rows(key, B, nrows, rows, wa, wb, mu, u_a, u_b, s, mode, guard);
}

}  // namespace tfhe_amd

using namespace tfhe_amd;

// ------------------------------------------------------------------ context

uint64_t next_context_uid() {
    static std::atomic<uint64_t> n{1};
    return n.fetch_add(1, std::memory_order_relaxed);
}

TraceScope::TraceScope(TfheAmdContext *c) : prev(g_trace) {
    if (!prev && c) {
        c->last_kernels.clear();
        g_trace = &c->last_kernels;
    }
}
TraceScope::~TraceScope() {
    if (!prev) g_trace = nullptr;
}

static int free_key(DeviceKey &k) {
    DeviceScope dev_scope(k.device);
    if (k.bk_ntt) (void)hipFree(k.bk_ntt);
    if (k.bk_v2) (void)hipFree(k.bk_v2);
    if (k.bk_fft) (void)hipFree(k.bk_fft);
    if (k.tw6) (void)hipFree(k.tw6);
    if (k.tw2) (void)hipFree(k.tw2);
    if (k.tw4) (void)hipFree(k.tw4);
    if (k.ksk) (void)hipFree(k.ksk);
    if (k.ksk4) (void)hipFree(k.ksk4);
    if (k.ksk5) (void)hipFree(k.ksk5);
    if (k.tables) (void)hipFree(k.tables);
    k = DeviceKey();
    return 0;
}

static int free_scratch(TfheAmdContext *c) {
    if (c->mtab) (void)hipFree(c->mtab);
    c->mtab = nullptr;
    c->mtab_bytes = 0;
    if (c->u_a) (void)hipFree(c->u_a);
    if (c->u_b) (void)hipFree(c->u_b);
    if (c->io) (void)hipFree(c->io);
    if (c->h_io) (void)hipHostFree(c->h_io);
    if (c->gflags) (void)hipFree(c->gflags);
    c->u_a = c->u_b = c->io = c->h_io = nullptr;
    c->gflags = nullptr;
    c->cap = 0;
    return 0;
}

int tfhe_amd_reserve(TfheAmdContext *c, int B) {
    if (!c || B < 0) return TFHE_AMD_E_ARG;
    if (B <= c->cap) return TFHE_AMD_OK;
    int cap = c->cap ? c->cap : 64;
    while (cap < B) cap *= 2;
    DeviceScope dev_scope(c->device);
    HIPCHK(dev_scope.rc);
    HIPCHK(hipDeviceSynchronize());   // the scratch may still be in use on a caller's stream
    free_scratch(c);
    HIPCHK(hipMalloc(&c->u_a, sizeof(int32_t) * 2 * (size_t)cap * kN));
    HIPCHK(hipMalloc(&c->u_b, sizeof(int32_t) * 2 * (size_t)cap));
    HIPCHK(hipMalloc(&c->io, sizeof(int32_t) * io_words(cap)));
    HIPCHK(hipMalloc(&c->gflags, sizeof(uint32_t) * 4 * (size_t)cap));
    HIPCHK(hipHostMalloc(&c->h_io, sizeof(int32_t) * io_words(cap), hipHostMallocDefault));
    c->cap = cap;
    return TFHE_AMD_OK;
}

// Upload: bk [kn][4][2][kN] (nullable: KS-only context), ksk [kN][8][4][kn+1]
static int context_init(TfheAmdContext *c, const int32_t *bk, const int32_t *ksk, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TFHE_AMD_E_NODEVICE;
    if (device < 0 || device >= ndev) return TFHE_AMD_E_ARG;
    c->device = device;
    c->key.device = device;
    DeviceScope dev_scope(device);
    HIPCHK(dev_scope.rc);
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipMalloc(&c->gstats, sizeof(uint32_t) * 4));
    HIPCHK(hipMemset(c->gstats, 0, sizeof(uint32_t) * 4));

    NttTables *ht = new NttTables;
    build_ntt_tables(ht);
    HIPCHK(hipMalloc(&c->key.tables, sizeof(NttTables)));
    HIPCHK(hipMemcpy(c->key.tables, ht, sizeof(NttTables), hipMemcpyHostToDevice));
    c->key.qinv_neg[0] = ht->qinv_neg[0];
    c->key.qinv_neg[1] = ht->qinv_neg[1];
    c->key.crt_h = ht->crt_h;
    c->key.crt_hp = ht->crt_hp;
    {
        std::vector<uint2> tw(kTw2Words);
        build_v2_twiddles(*ht, tw.data(), tw.data() + 32, tw.data() + 64, tw.data() + 64 + 2 * 27 * 64);
        HIPCHK(hipMalloc(&c->key.tw2, sizeof(uint2) * tw.size()));
        HIPCHK(hipMemcpy(c->key.tw2, tw.data(), sizeof(uint2) * tw.size(), hipMemcpyHostToDevice));
        std::vector<uint2> tw4(kTw4Words);
        build_v4_twiddles(*ht, tw4.data(), tw4.data() + 32, tw4.data() + 32 + 2 * 27 * 64);
        HIPCHK(hipMalloc(&c->key.tw4, sizeof(uint2) * tw4.size()));
        HIPCHK(hipMemcpy(c->key.tw4, tw4.data(), sizeof(uint2) * tw4.size(), hipMemcpyHostToDevice));
        std::vector<double2> tw6(kTw6Words);
        build_v6_twiddles(tw6.data());
        HIPCHK(hipMalloc(&c->key.tw6, sizeof(double2) * tw6.size()));
        HIPCHK(hipMemcpy(c->key.tw6, tw6.data(), sizeof(double2) * tw6.size(), hipMemcpyHostToDevice));
    }
    delete ht;

    if (bk) {
        const size_t coef_words = (size_t)kn * kKpl * 2 * kN;
        int32_t *d_coef = nullptr;
        HIPCHK(hipMalloc(&d_coef, sizeof(int32_t) * coef_words));
        HIPCHK(hipMemcpy(d_coef, bk, sizeof(int32_t) * coef_words, hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&c->key.bk_ntt, sizeof(uint32_t) * 2 * coef_words));
        HIPCHK(launch_bk_to_ntt(d_coef, c->key.bk_ntt, c->key.tables, c->stream));
        HIPCHK(hipMalloc(&c->key.bk_v2, sizeof(uint32_t) * 2 * coef_words));
        HIPCHK(launch_bk_v1_to_v2(c->key.bk_ntt, c->key.bk_v2, c->stream));
        HIPCHK(hipMalloc(&c->key.bk_fft, sizeof(double2) * (size_t)kn * kKpl * 2 * 512));
        HIPCHK(launch_bk_to_fft(d_coef, c->key.bk_fft, c->key.tw6, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(d_coef));
        // the v1-layout NTT key and the NTT tables only fed the v4 repack
        HIPCHK(hipFree(c->key.bk_ntt));
        c->key.bk_ntt = nullptr;
        HIPCHK(hipFree(c->key.tables));
        c->key.tables = nullptr;
        c->key.has_bk = true;
    }
    if (ksk) {
        // drop the zero digit h = 0 (lwe-keyswitch-functions.cu:919), pad rows to 512 words
        const size_t rows = (size_t)kN * kKsT * 3;
        std::vector<int32_t> packed(rows * kKsRow, 0);
        for (int i = 0; i < kN; i++)
            for (int j = 0; j < kKsT; j++)
                for (int h = 1; h < kKsBase; h++) {
                    const int32_t *src = ksk + (((size_t)i * kKsT + j) * kKsBase + h) * (kn + 1);
                    int32_t *dst = packed.data() + (((size_t)i * kKsT + j) * 3 + (h - 1)) * kKsRow;
                    memcpy(dst, src, sizeof(int32_t) * (kn + 1));
                }
        HIPCHK(hipMalloc(&c->key.ksk, sizeof(int32_t) * packed.size()));
        HIPCHK(hipMemcpy(c->key.ksk, packed.data(), sizeof(int32_t) * packed.size(), hipMemcpyHostToDevice));
        // batches above the small-batch kernel's range: the int8 MFMA key switch (ks-v5) or,
        // with TFHE_AMD_KS5=0, ks-v4; only the chosen layout is built
        if (ks5_enabled()) {
            HIPCHK(hipMalloc(&c->key.ksk5, sizeof(int32_t) * ksk_v5_words()));
            HIPCHK(launch_ksk_to_v5(c->key.ksk, c->key.ksk5, c->stream));
        } else {
            HIPCHK(hipMalloc(&c->key.ksk4, sizeof(int32_t) * ksk_v4_words()));
            HIPCHK(launch_ksk_to_v4(c->key.ksk, c->key.ksk4, c->stream));
        }
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return tfhe_amd_reserve(c, 64);
}

extern "C" int tfhe_amd_context_create_raw(const int32_t *bk, const int32_t *ksk, int device,
                                           TfheAmdContext **out) {
    if (!out || (!bk && !ksk)) return TFHE_AMD_E_ARG;
    TfheAmdContext *c = new TfheAmdContext();
    int rc = context_init(c, bk, ksk, device);
    if (rc != TFHE_AMD_OK) {
        tfhe_amd_context_destroy(c);
        *out = nullptr;
        return rc;
    }
    *out = c;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_context_destroy(TfheAmdContext *c) {
    if (!c) return TFHE_AMD_OK;
    tfhe_amd_internal_circuits_forget_context(c->uid);   // circuits' device state for this context
    DeviceScope dev_scope(c->device);
    (void)hipDeviceSynchronize();   // work on caller streams may still use the scratch
    for (auto &p : c->br_ev) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto &p : c->ks_ev) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    c->fence.release();
    for (hipEvent_t e : {c->ev_in, c->ev_out[0], c->ev_out[1]})
        if (e) (void)hipEventDestroy(e);
    if (c->copy_in) (void)hipStreamDestroy(c->copy_in);
    if (c->h_u) (void)hipHostFree(c->h_u);
    if (c->h_vout) (void)hipHostFree(c->h_vout);
    if (c->d_vout) (void)hipFree(c->d_vout);
    free_scratch(c);
    if (c->fa_tab) (void)hipFree(c->fa_tab);
    if (c->gstats) (void)hipFree(c->gstats);
    if (!c->shared_key) free_key(c->key);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return TFHE_AMD_OK;
}

// The four full-adder tables (tfhe_amd_full_add_table) on the context's device: 16 KB, made at the
// first tfhe_amd_full_add_batch_* call (or with a replica of a context that has them) and freed
// with the context.  Not key material: key_buffers below does not list them.
static int full_add_tables(TfheAmdContext *c) {
    if (c->fa_tab) return TFHE_AMD_OK;
    std::vector<int32_t> h((size_t)4 * kN);
    for (int e = 0; e < 4; ++e) tfhe_amd_full_add_table(h.data() + (size_t)e * kN, e >> 1, e & 1);
    DeviceScope dev_scope(c->device);
    HIPCHK(dev_scope.rc);
    HIPCHK(hipMalloc(&c->fa_tab, sizeof(int32_t) * h.size()));
    HIPCHK(hipMemcpy(c->fa_tab, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice));
    return TFHE_AMD_OK;
}

// The device buffers of a context's key, in a fixed order: (pointer, bytes) for each domain the
// context holds (replicas, digests)
static std::vector<std::pair<void **, size_t>> key_buffers(DeviceKey &k) {
    const size_t coef = (size_t)kn * kKpl * 2 * kN;
    return {{(void **)&k.bk_ntt, k.bk_ntt ? sizeof(uint32_t) * 2 * coef : 0},
            {(void **)&k.bk_v2, k.bk_v2 ? sizeof(uint32_t) * 2 * coef : 0},
            {(void **)&k.bk_fft, k.bk_fft ? sizeof(double2) * coef / 2 : 0},
            {(void **)&k.tw2, k.tw2 ? sizeof(uint2) * kTw2Words : 0},
            {(void **)&k.tw4, k.tw4 ? sizeof(uint2) * kTw4Words : 0},
            {(void **)&k.tw6, k.tw6 ? sizeof(double2) * kTw6Words : 0},
            {(void **)&k.ksk, k.ksk ? sizeof(int32_t) * kN * kKsT * 3 * kKsRow : 0},
            {(void **)&k.ksk4, k.ksk4 ? sizeof(int32_t) * ksk_v4_words() : 0},
            {(void **)&k.ksk5, k.ksk5 ? sizeof(int32_t) * ksk_v5_words() : 0},
            {(void **)&k.tables, k.tables ? sizeof(NttTables) : 0}};
}

// A context on `device` holding a copy of src's converted device key, copied device to device
// (key replicas device 0 -> peers): hipMemcpyPeerAsync runs over xGMI when the two
// GPUs have peer access (enabled here when the driver offers it) and is staged by HIP otherwise;
// ~180 MB per key instead of the host upload + on-device conversion of every replica.
extern "C" int tfhe_amd_context_create_replica(TfheAmdContext *src, int device, TfheAmdContext **out) {
    if (!src || !out) return TFHE_AMD_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return TFHE_AMD_E_ARG;
    TfheAmdContext *c = new TfheAmdContext();
    c->device = device;
    auto fail = [&](int rc) {
        tfhe_amd_context_destroy(c);
        return rc;
    };
    DeviceScope dev_scope(device);
    if (dev_scope.rc != hipSuccess) return fail(TFHE_AMD_E_HIP);
    if (device != src->device) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, device, src->device) == hipSuccess && can) {
            const hipError_t e = hipDeviceEnablePeerAccess(src->device, 0);
            if (e != hipSuccess) (void)hipGetLastError();   // already enabled: fine; otherwise HIP stages
        }
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->gstats, sizeof(uint32_t) * 4) != hipSuccess ||
        hipMemset(c->gstats, 0, sizeof(uint32_t) * 4) != hipSuccess)
        return fail(TFHE_AMD_E_HIP);
    // src's lock only while its pending work (the key conversions) drains and its key is snapshot:
    // the converted key is immutable from then on, so the peer copies below run without it and the
    // replicas of several slots (multi.cpp builds them from one worker per slot) copy concurrently
    DeviceKey src_key;
    {
        std::lock_guard<std::recursive_mutex> lk(src->mu);
        DeviceScope src_scope(src->device);
        if (hipStreamSynchronize(src->stream) != hipSuccess) return fail(TFHE_AMD_E_HIP);
        src_key = src->key;
    }
    DeviceKey &k = c->key;
    k = src_key;             // scalars (CRT constants, has_bk); pointers replaced below
    k.device = device;
    auto sb = key_buffers(src_key);
    auto db = key_buffers(k);
    for (size_t i = 0; i < db.size(); ++i) *db[i].first = nullptr;
    for (size_t i = 0; i < db.size(); ++i) {
        if (!sb[i].second) continue;
        if (hipMalloc(db[i].first, sb[i].second) != hipSuccess) return fail(TFHE_AMD_E_NOMEM);
        if (hipMemcpyPeerAsync(*db[i].first, device, *sb[i].first, src->device, sb[i].second, c->stream) != hipSuccess)
            return fail(TFHE_AMD_E_HIP);
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(TFHE_AMD_E_HIP);
    const int rc = tfhe_amd_reserve(c, 64);
    if (rc != TFHE_AMD_OK) return fail(rc);
    if (src->fa_tab && full_add_tables(c) != TFHE_AMD_OK) return fail(TFHE_AMD_E_HIP);   // a replica of a context that has them
    *out = c;
    return TFHE_AMD_OK;
}

// FNV-1a 64 over the context's device key buffers (key_buffers order), read back to the host:
// tests compare a replica's bytes with its source's
extern "C" int tfhe_amd_context_key_digest(TfheAmdContext *c, unsigned long long *digest) {
    if (!c || !digest) return TFHE_AMD_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceScope dev_scope(c->device);
    HIPCHK(dev_scope.rc);
    HIPCHK(hipStreamSynchronize(c->stream));
    uint64_t h = 1469598103934665603ull;
    std::vector<unsigned char> buf;
    for (auto &b : key_buffers(c->key)) {
        h = (h ^ (uint64_t)b.second) * 1099511628211ull;   // which domains are present, and their sizes
        if (!b.second) continue;
        buf.resize(b.second);
        HIPCHK(hipMemcpy(buf.data(), *b.first, b.second, hipMemcpyDeviceToHost));
        for (unsigned char x : buf) h = (h ^ x) * 1099511628211ull;
    }
    *digest = h;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_context_device(const TfheAmdContext *c) { return c ? c->device : -1; }

// device bytes held for the key material of a context (the key domains its kernels read)
extern "C" long long tfhe_amd_context_key_bytes(const TfheAmdContext *c) {
    if (!c) return TFHE_AMD_E_ARG;
    const DeviceKey &k = c->key;
    const long long bk = (long long)kn * kKpl * 2 * kN;   // coefficients per bootstrapping key
    long long n = 0;
    if (k.bk_ntt) n += bk * 2 * 4;
    if (k.bk_v2) n += bk * 2 * 4;
    if (k.bk_fft) n += bk / 2 * 16;
    if (k.tw2) n += (long long)kTw2Words * 8;
    if (k.tw4) n += (long long)kTw4Words * 8;
    if (k.tw6) n += (long long)kTw6Words * 16;
    if (k.ksk) n += (long long)kN * kKsT * 3 * kKsRow * 4;
    if (k.ksk4) n += (long long)ksk_v4_words() * 4;
    if (k.ksk5) n += (long long)ksk_v5_words() * 4;
    if (k.tables) n += (long long)sizeof(NttTables);
    return n;
}
extern "C" void *tfhe_amd_context_stream(TfheAmdContext *c) { return c ? (void *)c->stream : nullptr; }

extern "C" int tfhe_amd_sync(TfheAmdContext *c) {
    if (!c) return TFHE_AMD_E_ARG;
    DeviceScope dev_scope(c->device);
    HIPCHK(dev_scope.rc);
    HIPCHK(hipStreamSynchronize(c->stream));
    return TFHE_AMD_OK;
}

// ------------------------------------------------------------------ profiling

static void prof_collect(TfheAmdContext *c) {
    for (auto *vec : {&c->br_ev, &c->ks_ev}) {
        for (auto &p : *vec) {
            float ms = 0;
            (void)hipEventSynchronize(p.second);
            (void)hipEventElapsedTime(&ms, p.first, p.second);
            if (vec == &c->br_ev) { c->br_ms += ms; c->br_n++; }
            else { c->ks_ms += ms; c->ks_n++; }
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        vec->clear();
    }
}

extern "C" int tfhe_amd_profile_enable(TfheAmdContext *c, int enable) {
    if (!c) return TFHE_AMD_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceScope dev_scope(c->device);
    prof_collect(c);
    c->prof = enable != 0;
    c->br_ms = c->ks_ms = 0;
    c->br_n = c->ks_n = 0;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_profile_read(TfheAmdContext *c, double *br_ms, int *br_n, double *ks_ms, int *ks_n) {
    if (!c) return TFHE_AMD_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceScope dev_scope(c->device);
    prof_collect(c);
    if (br_ms) *br_ms = c->br_ms;
    if (br_n) *br_n = c->br_n;
    if (ks_ms) *ks_ms = c->ks_ms;
    if (ks_n) *ks_n = c->ks_n;
    return TFHE_AMD_OK;
}

// ------------------------------------------------------------------ batches

bool gate_spec(int gate, int32_t *c, int32_t *sa, int32_t *sb) {
    // constants of boot-gates.cu:98-397 (modSwitchToTorus32(+-1, 8) = +-2^29, (+-1, 4) = +-2^30)
    const int32_t e8 = 1 << 29, e4 = 1 << 30;
    switch (gate) {
    case TFHE_GATE_NAND:  *c = e8;  *sa = -1; *sb = -1; return true;
    case TFHE_GATE_OR:    *c = e8;  *sa = 1;  *sb = 1;  return true;
    case TFHE_GATE_AND:   *c = -e8; *sa = 1;  *sb = 1;  return true;
    case TFHE_GATE_XOR:   *c = e4;  *sa = 2;  *sb = 2;  return true;
    case TFHE_GATE_XNOR:  *c = -e4; *sa = -2; *sb = -2; return true;
    case TFHE_GATE_NOR:   *c = -e8; *sa = -1; *sb = -1; return true;
    case TFHE_GATE_ANDNY: *c = -e8; *sa = -1; *sb = 1;  return true;
    case TFHE_GATE_ANDYN: *c = -e8; *sa = 1;  *sb = -1; return true;
    case TFHE_GATE_ORNY:  *c = e8;  *sa = -1; *sb = 1;  return true;
    case TFHE_GATE_ORYN:  *c = e8;  *sa = 1;  *sb = -1; return true;
    default: return false;
    }
}

// The frame of the device entry points: B x halves blind rotations from in[0 .. halves) with mu into
// (u_a, u_b) — null: the context's scratch c->u_a / c->u_b — then, for n_ks > 0, the key switch of
// n_ks extracted samples into (res_a, res_b); halves = 2 is the MUX form, KS(u1 + u2 + (0, add_b)).
// `slots`: the ciphertext slots to reserve (guard flags per ciphertext, scratch samples per output).
// The callers have checked their arguments; the order lock -> device -> trace -> reserve (context.h
// EntryFrame) -> fence is what every entry point relies on.
static int batch_dev(TfheAmdContext *c, void *stream, int slots, int B, int halves, const BrInput *in, int32_t mu,
                     int32_t *u_a, int32_t *u_b, int n_ks = 0, int32_t add_b = 0, int32_t *res_a = nullptr,
                     int32_t *res_b = nullptr) {
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    EntryFrame frame(c, slots);
    if (frame.rc) return frame.rc;
    HIPCHK(c->fence.acquire(s));
    if (!u_a) {
        u_a = c->u_a;
        u_b = c->u_b;
    }
    {
        ProfScope ps(c, s, true);
        const Guard gd = ctx_guard(c);
        HIPCHK(run_br(c->key, B, halves, in, mu, u_a, u_b, s, &gd));
    }
    if (n_ks > 0) {
        ProfScope ps(c, s, false);   // (closes behind the fence's event, as the gate path's always did)
        HIPCHK(launch_keyswitch(c->key, n_ks, u_a, u_b, halves > 1 ? u_a + (size_t)B * kN : nullptr,
                                halves > 1 ? u_b + B : nullptr, add_b, res_a, res_b, s));
        HIPCHK(c->fence.done(s));
        return TFHE_AMD_OK;
    }
    HIPCHK(c->fence.done(s));
    return TFHE_AMD_OK;
}

// the same frame for entry points that live outside this file (engine.h ContextFrame)
int tfhe_amd_internal_frame(TfheAmdContext *c, void *stream, int u_slots, int (*fn)(const ContextFrame &, void *),
                            void *arg) {
    if (!c || !fn || u_slots < 0) return TFHE_AMD_E_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    EntryFrame frame(c, u_slots);
    if (frame.rc) return frame.rc;
    ContextFrame f{&c->key, c->device, s, nullptr, nullptr};
    if (u_slots == 0) return fn(f, arg);
    HIPCHK(c->fence.acquire(s));
    f.u_a = c->u_a;
    f.u_b = c->u_b;
    const int rc = fn(f, arg);
    HIPCHK(c->fence.done(s));
    return rc;
}

// batch_dev for entry points that live outside this file and bring their own BrInput (engine.h)
int tfhe_amd_internal_br_batch(TfheAmdContext *c, void *stream, int B, const BrInput *in, int32_t *u_a, int32_t *u_b,
                               int32_t *res_a, int32_t *res_b) {
    if (!c || !in || B <= 0 || !c->key.has_bk || (res_a && !c->key.ksk)) return TFHE_AMD_E_ARG;
    if (res_a) return batch_dev(c, stream, B, B, 1, in, 0, nullptr, nullptr, B, 0, res_a, res_b);
    return batch_dev(c, stream, B, B, 1, in, 0, u_a, u_b);
}

extern "C" int tfhe_amd_gate_batch_dev(TfheAmdContext *c, int gate, int B, int32_t *res_a, int32_t *res_b,
                                       const int32_t *ca_a, const int32_t *ca_b, const int32_t *cb_a,
                                       const int32_t *cb_b, const int32_t *cc_a, const int32_t *cc_b,
                                       void *stream) {
    if (!c || B < 0 || !c->key.has_bk || !c->key.ksk) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!res_a || !res_b || !ca_a || !ca_b || !cb_a || !cb_b) return TFHE_AMD_E_ARG;
    if (gate == TFHE_GATE_MUX) {
        if (!cc_a || !cc_b) return TFHE_AMD_E_ARG;
        // boot-gates.cu:407-448: u1 = woKS(-1/8 + a + b), u2 = woKS(-1/8 - a + c),
        // result = KS((0, 1/8) + u1 + u2)
        const BrInput in[2] = {{ca_a, ca_b, cb_a, cb_b, -kMu, 1, 1}, {ca_a, ca_b, cc_a, cc_b, -kMu, -1, 1}};
        return batch_dev(c, stream, B, B, 2, in, kMu, nullptr, nullptr, B, kMu, res_a, res_b);
    }
    BrInput in;
    if (!gate_spec(gate, &in.c, &in.sa, &in.sb)) return TFHE_AMD_E_ARG;
    in.x_a = ca_a; in.x_b = ca_b; in.y_a = cb_a; in.y_b = cb_b;
    return batch_dev(c, stream, B, B, 1, &in, kMu, nullptr, nullptr, B, 0, res_a, res_b);
}

extern "C" int tfhe_amd_bootstrap_woks_batch_dev(TfheAmdContext *c, int B, int32_t mu, const int32_t *x_a,
                                                 const int32_t *x_b, int32_t *u_a, int32_t *u_b, void *stream) {
    if (!c || B < 0 || !c->key.has_bk) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!x_a || !x_b || !u_a || !u_b) return TFHE_AMD_E_ARG;
    const BrInput in{x_a, x_b, nullptr, nullptr, 0, 1, 0};
    return batch_dev(c, stream, B, B, 1, &in, mu, u_a, u_b);   // (the guard flags live in the context's scratch)
}

extern "C" int tfhe_amd_bootstrap_batch_dev(TfheAmdContext *c, int B, int32_t mu, const int32_t *x_a,
                                            const int32_t *x_b, int32_t *res_a, int32_t *res_b, void *stream) {
    if (!c || B < 0 || !c->key.has_bk || !c->key.ksk) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!x_a || !x_b || !res_a || !res_b) return TFHE_AMD_E_ARG;
    const BrInput in{x_a, x_b, nullptr, nullptr, 0, 1, 0};
    return batch_dev(c, stream, B, B, 1, &in, mu, nullptr, nullptr, B, 0, res_a, res_b);
}

// ------------------------------------------------------------------ programmable bootstrapping

extern "C" int tfhe_amd_lut_fill(int32_t *tv, int p, const int32_t *values) {
    if (!tv || !values || p < 1 || p > kN || (p & (p - 1))) return TFHE_AMD_E_ARG;
    for (int j = 0; j < kN; ++j) tv[j] = values[(int)(((long)j * p) >> kLogN)];   // floor(j p / N)
    return TFHE_AMD_OK;
}

// many-LUT test vector: function j mod nu at coefficient j, zero where
// j mod nu >= n_fn
extern "C" int tfhe_amd_lut_fill_many(int32_t *tv, int p, int log_nu, int n_fn, const int32_t *values) {
    if (!tv || !values || p < 1 || p > kN || (p & (p - 1)) || log_nu < 0 || log_nu > 4) return TFHE_AMD_E_ARG;
    const int nu = 1 << log_nu;
    if (n_fn < 1 || n_fn > nu || (long)p * nu > kN) return TFHE_AMD_E_ARG;
    for (int j = 0; j < kN; ++j) {
        const int f = j & (nu - 1);
        tv[j] = f < n_fn ? values[(size_t)f * p + (int)(((long)j * p) >> kLogN)] : 0;
    }
    return TFHE_AMD_OK;
}

// B bootstraps of (0, c) + sa X + sb Y through the tables tv [n_lut][kN] (engine.h BrInput); ks:
// followed by the key switch into out (n = 500), else out is the extracted sample (N = 1024).
// n_out >= 1: the many-LUT form (engine.h BrInput), n_out B samples out, function-major; n_out = 0:
// the single-table form
static int lut_batch_dev(TfheAmdContext *c, bool ks, int B, int n_lut, const int32_t *tv, const int32_t *lut_index,
                         int32_t cst, int32_t sa, const int32_t *x_a, const int32_t *x_b, int32_t sb,
                         const int32_t *y_a, const int32_t *y_b, int32_t *out_a, int32_t *out_b, void *stream,
                         int log_nu = 0, int n_out = 0, int32_t sc = 0, const int32_t *z_a = nullptr,
                         const int32_t *z_b = nullptr) {
    if (!c || B < 0 || n_lut <= 0 || !tv || !c->key.has_bk || (ks && !c->key.ksk)) return TFHE_AMD_E_ARG;
    if (n_out != 0 && !many_args_ok(log_nu, n_out)) return TFHE_AMD_E_ARG;
    const int n_res = n_out ? n_out : 1;
    if ((long)B * n_res > 0x3fffffffL) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!x_a || !x_b || !out_a || !out_b || (sb && (!y_a || !y_b)) || (sc && (!z_a || !z_b))) return TFHE_AMD_E_ARG;
    const BrInput in{x_a, x_b, sb ? y_a : nullptr, sb ? y_b : nullptr, cst, sa, sb, n_lut, tv, lut_index, log_nu, n_out,
                     sc ? z_a : nullptr, sc ? z_b : nullptr, sc};
    // guard flags (per ciphertext) and the extracted samples (per output) live in the context's scratch
    if (ks) return batch_dev(c, stream, B * n_res, B, 1, &in, 0, nullptr, nullptr, B * n_res, 0, out_a, out_b);
    return batch_dev(c, stream, B * n_res, B, 1, &in, 0, out_a, out_b);
}

extern "C" int tfhe_amd_bootstrap_lut_many_woks_batch_dev(TfheAmdContext *c, int B, int n_lut, const int32_t *tv,
                                                          const int32_t *lut_index, int log_nu, int n_out,
                                                          int32_t cst, int32_t sa, const int32_t *x_a,
                                                          const int32_t *x_b, int32_t sb, const int32_t *y_a,
                                                          const int32_t *y_b, int32_t *u_a, int32_t *u_b,
                                                          void *stream) {
    if (!many_args_ok(log_nu, n_out)) return TFHE_AMD_E_ARG;
    return lut_batch_dev(c, false, B, n_lut, tv, lut_index, cst, sa, x_a, x_b, sb, y_a, y_b, u_a, u_b, stream, log_nu,
                         n_out);
}
extern "C" int tfhe_amd_bootstrap_lut_many_batch_dev(TfheAmdContext *c, int B, int n_lut, const int32_t *tv,
                                                     const int32_t *lut_index, int log_nu, int n_out, int32_t cst,
                                                     int32_t sa, const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                                     const int32_t *y_a, const int32_t *y_b, int32_t *res_a,
                                                     int32_t *res_b, void *stream) {
    if (!many_args_ok(log_nu, n_out)) return TFHE_AMD_E_ARG;
    return lut_batch_dev(c, true, B, n_lut, tv, lut_index, cst, sa, x_a, x_b, sb, y_a, y_b, res_a, res_b, stream,
                         log_nu, n_out);
}

// One-rotation full adders: B cells on half-torus bits, (0, -(k - 1)/16) + a + b
// (+ c) through the context's table for (enc_sum, enc_carry): one many-LUT launch (log_nu = 1,
// n_out = 2) and one key switch over the 2 B samples
extern "C" int tfhe_amd_full_add_batch_dev(TfheAmdContext *c, int B, int enc_sum, int enc_carry, const int32_t *a_a,
                                           const int32_t *a_b, const int32_t *b_a, const int32_t *b_b,
                                           const int32_t *c_a, const int32_t *c_b, int32_t *res_a, int32_t *res_b,
                                           void *stream) {
    if (!full_add_args_ok(c, B, enc_sum, enc_carry, c_a, c_b) || !c->key.has_bk || !c->key.ksk) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!a_a || !a_b || !b_a || !b_b || !res_a || !res_b) return TFHE_AMD_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const int rc = full_add_tables(c);
    if (rc) return rc;
    const int k = c_a ? 3 : 2;
    return lut_batch_dev(c, true, B, 1, c->fa_tab + (size_t)(2 * enc_sum + enc_carry) * kN, nullptr,
                         -(k - 1) * (1 << 28), 1, a_a, a_b, 1, b_a, b_b, res_a, res_b, stream, 1, 2, c_a ? 1 : 0, c_a,
                         c_b);
}

extern "C" int tfhe_amd_bootstrap_lut_woks_batch_dev(TfheAmdContext *c, int B, int n_lut, const int32_t *tv,
                                                     const int32_t *lut_index, int32_t cst, int32_t sa,
                                                     const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                                     const int32_t *y_a, const int32_t *y_b, int32_t *u_a,
                                                     int32_t *u_b, void *stream) {
    return lut_batch_dev(c, false, B, n_lut, tv, lut_index, cst, sa, x_a, x_b, sb, y_a, y_b, u_a, u_b, stream);
}
extern "C" int tfhe_amd_bootstrap_lut_batch_dev(TfheAmdContext *c, int B, int n_lut, const int32_t *tv,
                                                const int32_t *lut_index, int32_t cst, int32_t sa,
                                                const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                                const int32_t *y_a, const int32_t *y_b, int32_t *res_a,
                                                int32_t *res_b, void *stream) {
    return lut_batch_dev(c, true, B, n_lut, tv, lut_index, cst, sa, x_a, x_b, sb, y_a, y_b, res_a, res_b, stream);
}

extern "C" int tfhe_amd_keyswitch_batch_dev(TfheAmdContext *c, int B, const int32_t *u_a, const int32_t *u_b,
                                            int32_t *res_a, int32_t *res_b, void *stream) {
    if (!c || B < 0 || !c->key.ksk) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!u_a || !u_b || !res_a || !res_b) return TFHE_AMD_E_ARG;
    // k_keyswitch_v4 / k_keyswitch_v5 read u_a as uint4: the one caller pointer with an alignment
    // rule (include/tfhe_amd.h); every other entry point hands them the library's own scratch
    if (reinterpret_cast<uintptr_t>(u_a) % 16) return TFHE_AMD_E_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    EntryFrame frame(c, 0);
    if (frame.rc) return frame.rc;
    ProfScope ps(c, s, false);
    HIPCHK(launch_keyswitch(c->key, B, u_a, u_b, nullptr, nullptr, 0, res_a, res_b, s));
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_blind_rotate_dev(TfheAmdContext *c, int B, int iters, int32_t *acc, const int32_t *bara,
                                         void *stream) {
    if (!c || B < 0 || iters < 0 || iters > kn || !c->key.has_bk) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!acc || (iters > 0 && !bara)) return TFHE_AMD_E_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    EntryFrame frame(c, 0);
    if (frame.rc) return frame.rc;
    ProfScope ps(c, s, true);
    const int v = br_version();
    HIPCHK(v == 4 ? launch_blind_rotate_v4_debug(c->key, B, iters, acc, bara, s)
                  : launch_blind_rotate_v6_debug(c->key, B, iters, acc, bara, s));
    return TFHE_AMD_OK;
}

// tGswFFTExternMulToTLwe (tgsw-fft-operations.cu:124-264) for B accumulators acc [B][2][kN] with
// key indices key_index [B] (device arrays): acc <- BK_i (x) acc, exact (v4 arithmetic)
extern "C" int tfhe_amd_external_product_dev(TfheAmdContext *c, int B, const int32_t *key_index, int32_t *acc,
                                             void *stream) {
    if (!c || B < 0 || !c->key.has_bk) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!key_index || !acc) return TFHE_AMD_E_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    EntryFrame frame(c, 0);
    if (frame.rc) return frame.rc;
    HIPCHK(launch_external_product_v4(c->key, B, key_index, acc, s));
    return TFHE_AMD_OK;
}

// The L1 entry points of the TFHE API on host data (tier1.cpp): op 0 = external product
// (arg = key indices [B]), op 1 = tfhe_blindRotate_FFT (arg = bara [B][iters], the exact v4 CMux
// steps, skipping a_i = 0 as lwe-bootstrapping-functions-fft.cu:705); acc [B][2][kN] in place.
int tfhe_amd_internal_l1(TfheAmdContext *c, int op, int B, int iters, const int32_t *arg, int32_t *acc) {
    if (!c || B <= 0 || !arg || !acc || !c->key.has_bk || (op == 1 && (iters < 0 || iters > kn))) return TFHE_AMD_E_ARG;
    EntryFrame frame(c, 0);
    if (frame.rc) return frame.rc;
    const size_t na = op == 0 ? (size_t)B : (size_t)B * (size_t)(iters > 0 ? iters : 1);
    int32_t *d_acc = nullptr, *d_arg = nullptr;
    HIPCHK(hipMalloc(&d_acc, sizeof(int32_t) * 2 * kN * (size_t)B));
    if (hipMalloc(&d_arg, sizeof(int32_t) * na) != hipSuccess) {
        (void)hipFree(d_acc);
        return TFHE_AMD_E_NOMEM;
    }
    hipError_t e = hipMemcpyAsync(d_acc, acc, sizeof(int32_t) * 2 * kN * (size_t)B, hipMemcpyHostToDevice, c->stream);
    const size_t arg_words = op == 0 ? (size_t)B : (size_t)B * iters;
    if (e == hipSuccess && arg_words)
        e = hipMemcpyAsync(d_arg, arg, sizeof(int32_t) * arg_words, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = op == 0 ? launch_external_product_v4(c->key, B, d_arg, d_acc, c->stream)
                    : launch_blind_rotate_v4_debug(c->key, B, iters, d_acc, d_arg, c->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(acc, d_acc, sizeof(int32_t) * 2 * kN * (size_t)B, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_acc);
    (void)hipFree(d_arg);
    HIPCHK(e);
    return TFHE_AMD_OK;
}

int tfhe_amd_internal_device_cus(int device) {
    static std::atomic<int> cus[64];   // per device; concurrent first calls store the same value
    const bool cached = device >= 0 && device < 64;   // an out-of-range index is queried, never cached
    int n = cached ? cus[device].load(std::memory_order_relaxed) : 0;
    if (!n) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            n = 256;
        }
        if (cached) cus[device].store(n, std::memory_order_relaxed);
    }
    return n;
}

// device copy of host data on a context's GPU (tier1.cpp: the KSK row variances)
int tfhe_amd_internal_upload(TfheAmdContext *c, const void *host, size_t bytes, void **dev) {
    if (!c || !host || !dev) return TFHE_AMD_E_ARG;
    DeviceScope dev_scope(c->device);
    HIPCHK(dev_scope.rc);
    HIPCHK(hipMalloc(dev, bytes));
    HIPCHK(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
    return TFHE_AMD_OK;
}
void tfhe_amd_internal_free(int device, void *dev) {
    if (!dev) return;
    DeviceScope dev_scope(device);
    (void)hipFree(dev);
}

// a second context on the same GPU sharing `primary`'s key (own stream + scratch):
// used for per-thread lanes of the Tier-1 API
TfheAmdContext *tfhe_amd_context_lane(TfheAmdContext *primary) {
    TfheAmdContext *c = new TfheAmdContext();
    c->device = primary->device;
    c->key = primary->key;
    c->shared_key = true;
    DeviceScope dev_scope(c->device);
    if (dev_scope.rc != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->gstats, sizeof(uint32_t) * 4) != hipSuccess ||
        hipMemset(c->gstats, 0, sizeof(uint32_t) * 4) != hipSuccess ||
        tfhe_amd_reserve(c, 64) != TFHE_AMD_OK) {
        tfhe_amd_context_destroy(c);
        return nullptr;
    }
    return c;
}

// circuit.cpp
int tfhe_amd_circuit_run_dev_impl(uint64_t ctx_uid, const DeviceKey &key, int device, hipStream_t s,
                                  TfheAmdCircuit *c, int B, int32_t *wa, int32_t *wb, uint32_t *guard_stats);

extern "C" int tfhe_amd_circuit_run_dev(TfheAmdContext *c, TfheAmdCircuit *circ, int B, int32_t *wires_a,
                                        int32_t *wires_b, void *stream) {
    if (!c || !circ || B < 0 || !c->key.has_bk || !(c->key.ksk4 || c->key.ksk5)) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!wires_a || !wires_b) return TFHE_AMD_E_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    EntryFrame frame(c, 0);
    if (frame.rc) return frame.rc;
    return tfhe_amd_circuit_run_dev_impl(c->uid, c->key, c->device, s, circ, B, wires_a, wires_b, c->gstats);
}

extern "C" int tfhe_amd_set_guard_threshold(double distance) {
    // stricter than the default only: a threshold above 1/8 would let a rounding error of up to
    // 1 - threshold escape
    if (!(distance >= 0.0 && distance <= 0.125)) return TFHE_AMD_E_ARG;
    uint64_t bits;
    memcpy(&bits, &distance, 8);
    g_guard_hi.store((uint32_t)(bits >> 32));
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_guard_stats(TfheAmdContext *c, double *max_distance, long long *recomputed, int reset) {
    if (!c || !c->gstats) return TFHE_AMD_E_ARG;
    DeviceScope dev_scope(c->device);
    HIPCHK(dev_scope.rc);
    HIPCHK(hipDeviceSynchronize());   // launches on caller streams update the counters
    uint32_t h[4];
    HIPCHK(hipMemcpy(h, c->gstats, sizeof h, hipMemcpyDeviceToHost));
    if (max_distance) {
        const uint64_t bits = (uint64_t)h[1] << 32;   // high word: the distance rounded down
        double d;
        memcpy(&d, &bits, 8);
        *max_distance = d;
    }
    if (recomputed) *recomputed = h[0];
    if (reset) HIPCHK(hipMemset(c->gstats, 0, sizeof h));
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_last_kernels(TfheAmdContext *c, char *buf, int cap) {
    if (!c || !buf || cap <= 0) return TFHE_AMD_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const size_t n = std::min(c->last_kernels.size(), (size_t)cap - 1);
    memcpy(buf, c->last_kernels.data(), n);
    buf[n] = 0;
    return (int)c->last_kernels.size();
}

extern "C" int tfhe_amd_select_kernel(int br_version) {
    if (!br_available(br_version)) return TFHE_AMD_E_ARG;
    g_br_version.store(br_version);
    return TFHE_AMD_OK;
}

extern "C" const char *tfhe_amd_version(void) {
    // one immutable string per (blind-rotation, key-switch) generation pair
    static char names[8][6][48];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int b = 0; b <= 7; b++)
            for (int k = 1; k <= 5; k++) {
                if (b == 0 || b >= 6)
                    snprintf(names[b][k], sizeof names[b][k], "tfhe_amd gfx950 fft64 br-v%d ks-v%d", 6, k);
                else snprintf(names[b][k], sizeof names[b][k], "tfhe_amd gfx950 ntt2x27 br-v%d ks-v%d", b, k);
            }
    });
    return names[br_version()][ks_version()];
}
