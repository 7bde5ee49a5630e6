// acc.cpp — bootstrap from encrypted accumulators of the batched C ABI (include/tfhe_amd.h,
// DESIGN.md §3.8): the box fill, the blind rotation that starts from a TLWE sample, and the p-way
// selection composed of the function-major pack, the box fill, that rotation and the key switch.
// Argument checks, the accumulator scratch of the pack key and the host staging live here; the
// kernels are k_tlwe_box_fill (tlwe_box_fill.hip), the tlwe instantiations of the blind rotation
// (BrInput.acc) and the pack kernels (pack_v4.hip).  It reaches a context only through
// tfhe_amd_internal_frame and tfhe_amd_internal_br_batch (engine.h).
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

constexpr size_t kDigWords = (size_t)kn * kN;   // digit scratch of one output (pack.cpp)
constexpr size_t kAccWords = (size_t)2 * kN;    // one TLWE sample

// temporary device buffers of the host forms, freed on every path
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
    // a device copy of `words` host words, enqueued on s
    hipError_t put(const int32_t **out, const int32_t *host, size_t words, hipStream_t s) {
        int32_t *d = nullptr;
        hipError_t e = get(&d, words);
        if (e == hipSuccess) e = hipMemcpyAsync(d, host, sizeof(int32_t) * words, hipMemcpyHostToDevice, s);
        *out = d;
        return e;
    }
};

// ------------------------------------------------------------------ box fill

struct FillJob {
    int T, log_w;
    const int32_t *in;
    int32_t *out;
};

int fill_args(TfheAmdContext *c, const FillJob &j) {   // 1: nothing to do
    if (!c || j.T < 0 || j.log_w < 0 || j.log_w > kLogN || (long)j.T > 0x3fffffffL) return TFHE_AMD_E_ARG;
    if (j.T == 0) return 1;
    if (!j.in || !j.out) return TFHE_AMD_E_ARG;
    return TFHE_AMD_OK;
}

int fill_in_frame(const ContextFrame &f, void *arg) {
    const FillJob &j = *static_cast<FillJob *>(arg);
    HIPCHK(launch_tlwe_box_fill(j.T, j.log_w, j.in, j.out, f.stream));
    return TFHE_AMD_OK;
}

int fill_host_in_frame(const ContextFrame &f, void *arg) {
    const FillJob &j = *static_cast<FillJob *>(arg);
    hipStream_t s = f.stream;
    const size_t words = (size_t)j.T * kAccWords;
    DevBufs bufs;
    int32_t *d = nullptr;
    HIPCHK(bufs.get(&d, words));
    hipError_t e = hipMemcpyAsync(d, j.in, sizeof(int32_t) * words, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_tlwe_box_fill(j.T, j.log_w, d, d, s);
    if (e == hipSuccess) e = hipMemcpyAsync(j.out, d, sizeof(int32_t) * words, hipMemcpyDeviceToHost, s);
    const hipError_t w = hipStreamSynchronize(s);   // before the buffer goes, whatever happened
    HIPCHK(e);
    HIPCHK(w);
    return TFHE_AMD_OK;
}

// ------------------------------------------------------------------ bootstrap from an accumulator

struct AccJob {
    TfheAmdContext *c;
    bool ks;
    int B, n_acc;
    const int32_t *acc, *acc_index;
    int32_t cst, sa;
    const int32_t *x_a, *x_b;
    int32_t sb;
    const int32_t *y_a, *y_b;
    int32_t *out_a, *out_b;
};

// the argument rules shared by the device and host forms (no array is read); 1: nothing to do
int acc_args(const AccJob &j) {
    if (!j.c || j.B < 0 || j.n_acc <= 0 || !j.acc || (long)j.B > 0x3fffffffL) return TFHE_AMD_E_ARG;
    if (!j.acc_index && j.n_acc != 1 && j.n_acc != j.B && j.B > 0) return TFHE_AMD_E_ARG;
    if (j.B == 0) return 1;
    if (!j.x_a || !j.x_b || !j.out_a || !j.out_b || (j.sb && (!j.y_a || !j.y_b))) return TFHE_AMD_E_ARG;
    return TFHE_AMD_OK;
}

BrInput acc_input(const AccJob &j) {
    BrInput in{j.x_a, j.x_b, j.sb ? j.y_a : nullptr, j.sb ? j.y_b : nullptr, j.cst, j.sa, j.sb};
    in.acc = j.acc;
    in.acc_index = j.acc_index;
    in.n_acc = j.n_acc;
    return in;
}

int acc_dev(const AccJob &j, void *stream) {
    const BrInput in = acc_input(j);
    // (the guard flags, and the extracted samples of the key-switched form, live in the context's scratch)
    return tfhe_amd_internal_br_batch(j.c, stream, j.B, &in, j.ks ? nullptr : j.out_a, j.ks ? nullptr : j.out_b,
                                      j.ks ? j.out_a : nullptr, j.ks ? j.out_b : nullptr);
}

int acc_host_in_frame(const ContextFrame &f, void *arg) {
    const AccJob &j = *static_cast<AccJob *>(arg);
    if (!f.key->has_bk || (j.ks && !f.key->ksk)) return TFHE_AMD_E_ARG;
    hipStream_t s = f.stream;
    const size_t B = (size_t)j.B, row = j.ks ? kn : kN;
    DevBufs bufs;
    AccJob d = j;
    HIPCHK(bufs.put(&d.acc, j.acc, (size_t)j.n_acc * kAccWords, s));
    if (j.acc_index) HIPCHK(bufs.put(&d.acc_index, j.acc_index, B, s));
    HIPCHK(bufs.put(&d.x_a, j.x_a, B * kn, s));
    HIPCHK(bufs.put(&d.x_b, j.x_b, B, s));
    if (j.sb) {
        HIPCHK(bufs.put(&d.y_a, j.y_a, B * kn, s));
        HIPCHK(bufs.put(&d.y_b, j.y_b, B, s));
    }
    HIPCHK(bufs.get(&d.out_a, B * row));
    HIPCHK(bufs.get(&d.out_b, B));
    hipError_t e = hipSuccess;
    const int rc = acc_dev(d, s);
    if (rc == TFHE_AMD_OK) {
        e = hipMemcpyAsync(j.out_a, d.out_a, sizeof(int32_t) * B * row, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(j.out_b, d.out_b, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s);
    }
    const hipError_t w = hipStreamSynchronize(s);   // before the buffers go, whatever happened
    if (rc != TFHE_AMD_OK) return rc;
    HIPCHK(e);
    HIPCHK(w);
    return TFHE_AMD_OK;
}

int acc_host(const AccJob &j) {
    const int rc = acc_args(j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    if (j.acc_index)   // the host form refuses what the device form clamps
        for (int i = 0; i < j.B; ++i)
            if (j.acc_index[i] < 0 || j.acc_index[i] >= j.n_acc) return TFHE_AMD_E_ARG;
    AccJob h = j;
    // the outer frame holds the context (the lock is recursive) from the uploads to the read-back
    return tfhe_amd_internal_frame(j.c, nullptr, 0, acc_host_in_frame, &h);
}

// ------------------------------------------------------------------ p-way selection

struct SelectJob {
    TfheAmdContext *c;
    TfheAmdPackKey *key;
    int B, p;
    const int32_t *cand_a, *cand_b;
    int32_t cst, sa;
    const int32_t *y_a, *y_b;
    int32_t *res_a, *res_b;
};

int log2_exact(int p) {   // -1 unless p is a power of two
    int l = 0;
    while ((1 << l) < p) ++l;
    return (1 << l) == p ? l : -1;
}

int select_args(const SelectJob &j) {   // 1: nothing to do
    if (!j.c || !j.key || !j.key->v2 || j.B < 0 || (long)j.B > 0x3fffffffL) return TFHE_AMD_E_ARG;
    if (j.key->device != tfhe_amd_context_device(j.c)) return TFHE_AMD_E_ARG;
    if (j.p < 2 || j.p > kN || log2_exact(j.p) < 0) return TFHE_AMD_E_ARG;
    if (j.B == 0) return 1;
    if (!j.cand_a || !j.cand_b || !j.y_a || !j.y_b || !j.res_a || !j.res_b) return TFHE_AMD_E_ARG;
    return TFHE_AMD_OK;
}

// pack (function-major candidates -> one sample per query, value m at m N / p) -> box fill -> the
// rotation of sample q by selector q -> key switch.  The key's scratch holds the digits of one pack
// batch and all B samples until the rotation (and the guard launch behind it) has read them.
int select_in_frame(const ContextFrame &f, void *arg) {
    const SelectJob &j = *static_cast<SelectJob *>(arg);
    if (!f.key->has_bk || !f.key->ksk) return TFHE_AMD_E_ARG;
    TfheAmdPackKey *key = j.key;
    hipStream_t s = f.stream;
    std::lock_guard<std::mutex> lock(key->mu);
    const size_t need_dig = (size_t)(j.B < kPackMaxBatch ? j.B : kPackMaxBatch), need_acc = (size_t)j.B;
    if (key->dig_outputs < need_dig || key->acc_outputs < need_acc) {
        HIPCHK(hipDeviceSynchronize());   // the scratch may still be in use on another stream
        if (key->dig_outputs < need_dig) {
            if (key->dig) (void)hipFree(key->dig);
            key->dig = nullptr;
            key->dig_outputs = 0;
            HIPCHK(hipMalloc(&key->dig, sizeof(uint32_t) * need_dig * kDigWords));
            key->dig_outputs = need_dig;
        }
        if (key->acc_outputs < need_acc) {
            if (key->acc) (void)hipFree(key->acc);
            key->acc = nullptr;
            key->acc_outputs = 0;
            HIPCHK(hipMalloc(&key->acc, sizeof(int32_t) * need_acc * kAccWords));
            key->acc_outputs = need_acc;
        }
    }
    HIPCHK(key->fence.acquire(s));
    const int log_p = log2_exact(j.p);
    for (int t0 = 0; t0 < j.B; t0 += kPackMaxBatch) {   // batches share the digit scratch in stream order
        const int Tc = j.B - t0 < kPackMaxBatch ? j.B - t0 : kPackMaxBatch;
        HIPCHK(launch_pack_fm(*f.key, key->v2, Tc, j.p, j.B, j.cand_a + (size_t)t0 * kn, j.cand_b + t0, kN >> log_p,
                              key->dig, pack_split(Tc, key->cus), key->acc + (size_t)t0 * kAccWords, s));
    }
    HIPCHK(launch_tlwe_box_fill(j.B, kLogN - log_p, key->acc, key->acc, s));
    BrInput in{j.y_a, j.y_b, nullptr, nullptr, j.cst, j.sa, 0};
    in.acc = key->acc;
    in.n_acc = j.B;
    const int rc = tfhe_amd_internal_br_batch(j.c, s, j.B, &in, nullptr, nullptr, j.res_a, j.res_b);
    HIPCHK(key->fence.done(s));   // whatever was enqueued is ordered before the scratch's next user
    return rc;
}

int select_host_in_frame(const ContextFrame &f, void *arg) {
    const SelectJob &j = *static_cast<SelectJob *>(arg);
    hipStream_t s = f.stream;
    const size_t B = (size_t)j.B, n_c = (size_t)j.p * B;
    DevBufs bufs;
    SelectJob d = j;
    HIPCHK(bufs.put(&d.cand_a, j.cand_a, n_c * kn, s));
    HIPCHK(bufs.put(&d.cand_b, j.cand_b, n_c, s));
    HIPCHK(bufs.put(&d.y_a, j.y_a, B * kn, s));
    HIPCHK(bufs.put(&d.y_b, j.y_b, B, s));
    HIPCHK(bufs.get(&d.res_a, B * kn));
    HIPCHK(bufs.get(&d.res_b, B));
    hipError_t e = hipSuccess;
    const int rc = tfhe_amd_internal_frame(j.c, s, 0, select_in_frame, &d);
    if (rc == TFHE_AMD_OK) {
        e = hipMemcpyAsync(j.res_a, d.res_a, sizeof(int32_t) * B * kn, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(j.res_b, d.res_b, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s);
    }
    const hipError_t w = hipStreamSynchronize(s);   // before the buffers go, whatever happened
    if (rc != TFHE_AMD_OK) return rc;
    HIPCHK(e);
    HIPCHK(w);
    return TFHE_AMD_OK;
}

}  // namespace

extern "C" int tfhe_amd_tlwe_box_fill_dev(TfheAmdContext *ctx, int T, int log_w, const int32_t *in, int32_t *out,
                                          void *stream) {
    FillJob j{T, log_w, in, out};
    const int rc = fill_args(ctx, j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    return tfhe_amd_internal_frame(ctx, stream, 0, fill_in_frame, &j);
}

extern "C" int tfhe_amd_tlwe_box_fill_host(TfheAmdContext *ctx, int T, int log_w, const int32_t *in, int32_t *out) {
    FillJob j{T, log_w, in, out};
    const int rc = fill_args(ctx, j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    return tfhe_amd_internal_frame(ctx, nullptr, 0, fill_host_in_frame, &j);
}

extern "C" int tfhe_amd_bootstrap_acc_woks_batch_dev(TfheAmdContext *ctx, int B, int n_acc, const int32_t *acc,
                                                     const int32_t *acc_index, int32_t c, int32_t sa,
                                                     const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                                     const int32_t *y_a, const int32_t *y_b, int32_t *u_a,
                                                     int32_t *u_b, void *stream) {
    const AccJob j{ctx, false, B, n_acc, acc, acc_index, c, sa, x_a, x_b, sb, y_a, y_b, u_a, u_b};
    const int rc = acc_args(j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    return acc_dev(j, stream);
}

extern "C" int tfhe_amd_bootstrap_acc_batch_dev(TfheAmdContext *ctx, int B, int n_acc, const int32_t *acc,
                                                const int32_t *acc_index, int32_t c, int32_t sa, const int32_t *x_a,
                                                const int32_t *x_b, int32_t sb, const int32_t *y_a,
                                                const int32_t *y_b, int32_t *res_a, int32_t *res_b, void *stream) {
    const AccJob j{ctx, true, B, n_acc, acc, acc_index, c, sa, x_a, x_b, sb, y_a, y_b, res_a, res_b};
    const int rc = acc_args(j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    return acc_dev(j, stream);
}

extern "C" int tfhe_amd_bootstrap_acc_woks_batch_host(TfheAmdContext *ctx, int B, int n_acc, const int32_t *acc,
                                                      const int32_t *acc_index, int32_t c, int32_t sa,
                                                      const int32_t *x_a, const int32_t *x_b, int32_t sb,
                                                      const int32_t *y_a, const int32_t *y_b, int32_t *u_a,
                                                      int32_t *u_b) {
    return acc_host(AccJob{ctx, false, B, n_acc, acc, acc_index, c, sa, x_a, x_b, sb, y_a, y_b, u_a, u_b});
}

extern "C" int tfhe_amd_bootstrap_acc_batch_host(TfheAmdContext *ctx, int B, int n_acc, const int32_t *acc,
                                                 const int32_t *acc_index, int32_t c, int32_t sa, const int32_t *x_a,
                                                 const int32_t *x_b, int32_t sb, const int32_t *y_a,
                                                 const int32_t *y_b, int32_t *res_a, int32_t *res_b) {
    return acc_host(AccJob{ctx, true, B, n_acc, acc, acc_index, c, sa, x_a, x_b, sb, y_a, y_b, res_a, res_b});
}

extern "C" int tfhe_amd_select_batch_dev(TfheAmdContext *ctx, TfheAmdPackKey *pack_key, int B, int p,
                                         const int32_t *cand_a, const int32_t *cand_b, int32_t c, int32_t sa,
                                         const int32_t *y_a, const int32_t *y_b, int32_t *res_a, int32_t *res_b,
                                         void *stream) {
    SelectJob j{ctx, pack_key, B, p, cand_a, cand_b, c, sa, y_a, y_b, res_a, res_b};
    const int rc = select_args(j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    return tfhe_amd_internal_frame(ctx, stream, 0, select_in_frame, &j);
}

extern "C" int tfhe_amd_select_batch_host(TfheAmdContext *ctx, TfheAmdPackKey *pack_key, int B, int p,
                                          const int32_t *cand_a, const int32_t *cand_b, int32_t c, int32_t sa,
                                          const int32_t *y_a, const int32_t *y_b, int32_t *res_a, int32_t *res_b) {
    SelectJob j{ctx, pack_key, B, p, cand_a, cand_b, c, sa, y_a, y_b, res_a, res_b};
    const int rc = select_args(j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    // the outer frame holds the context (the lock is recursive) from the uploads to the read-back
    return tfhe_amd_internal_frame(ctx, nullptr, 0, select_host_in_frame, &j);
}
