// pack.cpp — LWE -> TLWE packing key switch of the batched C ABI (include/tfhe_amd.h, DESIGN.md
// §3.7): the imported packing key, the argument checks, the digit scratch and the host staging.  The
// kernels are k_pack_digits / k_pack_v4 (pack_v4.hip, exact arithmetic).  It reaches a context only
// through tfhe_amd_internal_frame (engine.h).
#include <cstdio>
#include <mutex>
#include <vector>

#include "engine.h"
#include "pack_key.h"
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

constexpr size_t kGroupWords = (size_t)kKpl * 2 * kN;   // coefficient domain, one prime
constexpr size_t kDigWords = (size_t)kn * kN;           // digit scratch of one output

struct ImportJob {
    const int32_t *coef;
    TfheAmdPackKey *key;
};

// upload + the two conversion kernels of the bootstrapping key over the 750 groups (a group of 4
// rows x 2 polynomials has the shape of a TGSW sample); the import brings its own NTT tables
int import_in_frame(const ContextFrame &f, void *arg) {
    ImportJob &j = *static_cast<ImportJob *>(arg);
    const size_t words = (size_t)kPackGroups * kGroupWords;
    int32_t *d_coef = nullptr;
    uint32_t *d_ntt = nullptr;
    NttTables *d_tab = nullptr;
    NttTables *ht = new NttTables;
    build_ntt_tables(ht);
    hipError_t e = hipMalloc(&d_tab, sizeof(NttTables));
    if (e == hipSuccess) e = hipMemcpy(d_tab, ht, sizeof(NttTables), hipMemcpyHostToDevice);
    delete ht;
    if (e == hipSuccess) e = hipMalloc(&d_coef, sizeof(int32_t) * words);
    if (e == hipSuccess) e = hipMalloc(&d_ntt, sizeof(uint32_t) * 2 * words);
    if (e == hipSuccess) e = hipMalloc(&j.key->v2, sizeof(uint32_t) * 2 * words);
    if (e == hipSuccess) e = hipMemcpyAsync(d_coef, j.coef, sizeof(int32_t) * words, hipMemcpyHostToDevice, f.stream);
    if (e == hipSuccess) e = launch_tgsw_to_ntt(d_coef, d_ntt, d_tab, kPackGroups, f.stream);
    if (e == hipSuccess) e = launch_tgsw_v1_to_v2(d_ntt, j.key->v2, kPackGroups, f.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(f.stream);
    (void)hipFree(d_coef);
    (void)hipFree(d_ntt);
    (void)hipFree(d_tab);
    HIPCHK(e);
    HIPCHK(hipDeviceGetAttribute(&j.key->cus, hipDeviceAttributeMultiprocessorCount, f.device));
    j.key->device = f.device;
    return TFHE_AMD_OK;
}

struct PackJob {
    TfheAmdPackKey *key;
    int T, P;
    const int32_t *in_a, *in_b, *pos;
    int32_t *out;
};

// the argument rules shared by the device and host forms (no array is read); 1: nothing to do
int pack_args(TfheAmdContext *c, const TfheAmdPackKey *key, const PackJob &j) {
    if (!c || !key || !key->v2 || j.T < 0) return TFHE_AMD_E_ARG;
    if (key->device != tfhe_amd_context_device(c)) return TFHE_AMD_E_ARG;
    if (j.T == 0) return 1;
    if (j.P < 1 || j.P > kN || !j.in_a || !j.in_b || !j.out) return TFHE_AMD_E_ARG;
    return TFHE_AMD_OK;
}

int pack_in_frame(const ContextFrame &f, void *arg) {
    const PackJob &j = *static_cast<PackJob *>(arg);
    TfheAmdPackKey *key = j.key;
    hipStream_t s = f.stream;
    std::lock_guard<std::mutex> lock(key->mu);
    const size_t need = (size_t)(j.T < kPackMaxBatch ? j.T : kPackMaxBatch);
    if (key->dig_outputs < need) {
        HIPCHK(hipDeviceSynchronize());   // the scratch may still be in use on another stream
        if (key->dig) (void)hipFree(key->dig);
        key->dig = nullptr;
        key->dig_outputs = 0;
        HIPCHK(hipMalloc(&key->dig, sizeof(uint32_t) * need * kDigWords));
        key->dig_outputs = need;
    }
    HIPCHK(key->fence.acquire(s));
    for (int t0 = 0; t0 < j.T; t0 += kPackMaxBatch) {   // batches share the scratch in stream order
        const int Tc = j.T - t0 < kPackMaxBatch ? j.T - t0 : kPackMaxBatch;
        HIPCHK(launch_pack(*f.key, key->v2, Tc, j.P, j.in_a + (size_t)t0 * j.P * kn, j.in_b + (size_t)t0 * j.P, j.pos,
                           key->dig, pack_split(Tc, key->cus), j.out + (size_t)t0 * 2 * kN, s));
    }
    HIPCHK(key->fence.done(s));
    return TFHE_AMD_OK;
}

// temporary device buffers of the host form, freed on every path
struct DevBufs {
    std::vector<void *> p;
    ~DevBufs() {
        for (void *q : p) (void)hipFree(q);
    }
    template <class T>
    hipError_t get(T **out, size_t words) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, sizeof(T) * (words ? words : 1));
        if (e == hipSuccess) p.push_back(q);
        *out = static_cast<T *>(q);
        return e;
    }
};

struct HostPackJob {
    TfheAmdContext *c;
    PackJob j;   // host pointers
};

int pack_host_in_frame(const ContextFrame &f, void *arg) {
    HostPackJob &h = *static_cast<HostPackJob *>(arg);
    const PackJob &j = h.j;
    hipStream_t s = f.stream;
    const size_t n_in = (size_t)j.T * j.P, n_out = (size_t)j.T * 2 * kN;
    DevBufs bufs;
    int32_t *d_a, *d_b, *d_pos = nullptr, *d_out;
    HIPCHK(bufs.get(&d_a, n_in * kn));
    HIPCHK(bufs.get(&d_b, n_in));
    if (j.pos) HIPCHK(bufs.get(&d_pos, (size_t)j.P));
    HIPCHK(bufs.get(&d_out, n_out));
    HIPCHK(hipMemcpyAsync(d_a, j.in_a, sizeof(int32_t) * n_in * kn, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_b, j.in_b, sizeof(int32_t) * n_in, hipMemcpyHostToDevice, s));
    if (j.pos) HIPCHK(hipMemcpyAsync(d_pos, j.pos, sizeof(int32_t) * j.P, hipMemcpyHostToDevice, s));
    hipError_t sync = hipSuccess;
    PackJob d{j.key, j.T, j.P, d_a, d_b, d_pos, d_out};
    const int rc = tfhe_amd_internal_frame(h.c, s, 0, pack_in_frame, &d);
    if (rc == TFHE_AMD_OK) sync = hipMemcpyAsync(j.out, d_out, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, s);
    const hipError_t e = hipStreamSynchronize(s);   // before the buffers go, whatever happened
    if (rc != TFHE_AMD_OK) return rc;
    HIPCHK(sync);
    HIPCHK(e);
    return TFHE_AMD_OK;
}

}  // namespace

extern "C" int tfhe_amd_pack_key_import(TfheAmdContext *ctx, const int32_t *coef_host, TfheAmdPackKey **out) {
    if (out) *out = nullptr;
    if (!ctx || !out || !coef_host) return TFHE_AMD_E_ARG;
    TfheAmdPackKey *key = new TfheAmdPackKey();
    ImportJob j{coef_host, key};
    const int rc = tfhe_amd_internal_frame(ctx, nullptr, 0, import_in_frame, &j);
    if (rc != TFHE_AMD_OK) {
        if (key->v2) {
            DeviceScope dev_scope(tfhe_amd_context_device(ctx));
            (void)hipFree(key->v2);
        }
        delete key;
        return rc;
    }
    *out = key;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_pack_key_destroy(TfheAmdPackKey *key) {
    if (!key) return TFHE_AMD_OK;
    {
        DeviceScope dev_scope(key->device);
        (void)hipDeviceSynchronize();   // launches on caller streams may still read the key
        key->fence.release();
        if (key->dig) (void)hipFree(key->dig);
        if (key->acc) (void)hipFree(key->acc);
        if (key->v2) (void)hipFree(key->v2);
    }
    delete key;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_pack_dev(TfheAmdContext *ctx, TfheAmdPackKey *key, int T, int P, const int32_t *in_a,
                                 const int32_t *in_b, const int32_t *pos, int32_t *out, void *stream) {
    PackJob j{key, T, P, in_a, in_b, pos, out};
    const int rc = pack_args(ctx, key, j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    return tfhe_amd_internal_frame(ctx, stream, 0, pack_in_frame, &j);
}

extern "C" int tfhe_amd_pack_host(TfheAmdContext *ctx, TfheAmdPackKey *key, int T, int P, const int32_t *in_a,
                                  const int32_t *in_b, const int32_t *pos, int32_t *out) {
    HostPackJob h{ctx, {key, T, P, in_a, in_b, pos, out}};
    const int rc = pack_args(ctx, key, h.j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    if (pos) {   // the host form refuses what the device form drops or leaves unspecified
        bool seen[kN] = {};
        for (int p = 0; p < P; ++p) {
            if (pos[p] < 0 || pos[p] >= kN || seen[pos[p]]) return TFHE_AMD_E_ARG;
            seen[pos[p]] = true;
        }
    }
    // the outer frame holds the context (the lock is recursive) from the uploads to the read-back
    return tfhe_amd_internal_frame(ctx, nullptr, 0, pack_host_in_frame, &h);
}
