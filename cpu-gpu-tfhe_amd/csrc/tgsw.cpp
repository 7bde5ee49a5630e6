// tgsw.cpp — leveled mode of the batched C ABI (include/tfhe_amd.h): imported sets
// of caller-supplied TGSW samples, CMux batches and table lookups on them.  The kernels are
// k_tgsw_lookup_v4 / k_tgsw_cmux_v4 (blind_rotate_v4.hip, exact arithmetic); this file holds the
// sets, the argument checks, the CMux tree of the vertical packing and the host staging.  It
// reaches a context only through tfhe_amd_internal_frame (engine.h).
#include <cstdio>
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

constexpr size_t kSampleWords = (size_t)kKpl * 2 * kN;   // coefficient domain, one prime

struct ImportJob {
    int n;
    const int32_t *coef;
    TfheAmdTgsw *set;
};

// upload + the two conversion kernels of the bootstrapping key, over n samples; the context freed
// its device NttTables after its own key conversion, so the import brings its own
int import_in_frame(const ContextFrame &f, void *arg) {
    ImportJob &j = *static_cast<ImportJob *>(arg);
    const size_t words = (size_t)j.n * kSampleWords;
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
    if (e == hipSuccess) e = hipMalloc(&j.set->v2, sizeof(uint32_t) * 2 * words);
    if (e == hipSuccess) e = hipMemcpyAsync(d_coef, j.coef, sizeof(int32_t) * words, hipMemcpyHostToDevice, f.stream);
    if (e == hipSuccess) e = launch_tgsw_to_ntt(d_coef, d_ntt, d_tab, j.n, f.stream);
    if (e == hipSuccess) e = launch_tgsw_v1_to_v2(d_ntt, j.set->v2, j.n, f.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(f.stream);
    (void)hipFree(d_coef);
    (void)hipFree(d_ntt);
    (void)hipFree(d_tab);
    HIPCHK(e);
    j.set->device = f.device;
    j.set->count = j.n;
    return TFHE_AMD_OK;
}

int log2_exact(int v) {   // -1 unless v is a power of two
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

struct LookupJob {
    TfheAmdTgsw *set;
    bool ks;
    int B, d, n_tab, n_poly, tab_rows, log_stride, n_out;
    const int32_t *sel, *tab, *tab_index;
    int32_t *out_a, *out_b;
};

// shape checks shared by the device and host forms (no pointer is read)
bool lookup_shape_ok(const TfheAmdTgsw *set, int B, int d, int n_tab, int n_poly, int tab_rows, int log_stride,
                     int n_out) {
    const int lp = log2_exact(n_poly);
    if (!set || B < 0 || lp < 0 || lp > 4 || d < lp || n_tab < 1 || (tab_rows != 1 && tab_rows != 2)) return false;
    if (log_stride < 0 || (d - lp) + log_stride > kLogN) return false;
    if (n_out < 1 || n_out > 16 || n_out > (1 << log_stride)) return false;
    return (long)B * n_out <= 0x3fffffffL && (long)B * n_poly <= 0x3fffffffL;
}

const char *const kTreeLabel[4] = {"k_tgsw_cmux_v4(tree-level-0)", "k_tgsw_cmux_v4(tree-level-1)",
                                   "k_tgsw_cmux_v4(tree-level-2)", "k_tgsw_cmux_v4(tree-level-3)"};

int lookup_in_frame(const ContextFrame &f, void *arg) {
    const LookupJob &j = *static_cast<LookupJob *>(arg);
    TfheAmdTgsw *set = j.set;
    hipStream_t s = f.stream;
    if (j.ks && !f.key->ksk) return TFHE_AMD_E_ARG;
    const int levels = log2_exact(j.n_poly), d_h = j.d - levels;
    TgswLookup a;
    a.B = j.B;
    a.count = set->count;
    a.sel = j.sel;
    a.sel_stride = j.d;
    a.d_h = d_h;
    a.log_stride = j.log_stride;
    a.n_out = j.n_out;
    a.tab = j.tab;
    a.tab_stride = (long)j.tab_rows * kN;
    a.n_tab = j.n_tab;
    a.tab_rows = j.tab_rows;
    a.tab_index = j.tab_index;
    std::unique_lock<std::mutex> tree_lock(set->mu, std::defer_lock);
    if (levels > 0) {
        // address bits d_h .. d - 1 pick the polynomial: level l halves the candidates with bit d_h + l,
        // B n_poly / 2^(l + 1) pairs in one launch; the levels alternate between the two scratch halves
        tree_lock.lock();
        const size_t half = (size_t)j.B * (j.n_poly / 2) * 2 * kN;   // level 0's output, the largest
        const size_t need = half + half / 2;
        if (set->tree_words < need) {
            HIPCHK(hipDeviceSynchronize());   // the scratch may still be in use on another stream
            if (set->tree) (void)hipFree(set->tree);
            set->tree = nullptr;
            set->tree_words = 0;
            HIPCHK(hipMalloc(&set->tree, sizeof(int32_t) * need));
            set->tree_words = need;
        }
        HIPCHK(set->fence.acquire(s));
        int32_t *buf[2] = {set->tree, set->tree + half};
        for (int l = 0; l < levels; ++l) {
            TgswCmux c;
            c.count = set->count;
            c.sel = j.sel + d_h + l;
            c.sel_stride = j.d;
            c.ppq = j.n_poly >> (l + 1);
            c.out = buf[l & 1];
            if (l == 0) {   // the table itself, broadcast over the queries
                c.d0 = j.tab;
                c.n_poly = j.n_poly;
                c.rows = j.tab_rows;
                c.n_tab = j.n_tab;
                c.tab_index = j.tab_index;
            } else {
                c.d0 = buf[(l - 1) & 1];
                c.d1 = c.d0 + 2 * kN;
                c.pair_stride = 4 * kN;
            }
            HIPCHK(launch_tgsw_cmux_v4(*f.key, set->v2, j.B * c.ppq, c, s, kTreeLabel[l]));
        }
        a.tab = buf[(levels - 1) & 1];
        a.per_query = 1;
        a.tab_index = nullptr;
    }
    int32_t *u_a = j.ks ? f.u_a : j.out_a, *u_b = j.ks ? f.u_b : j.out_b;
    HIPCHK(launch_tgsw_lookup_v4(*f.key, set->v2, a, u_a, u_b, s));
    if (levels > 0) HIPCHK(set->fence.done(s));
    if (j.ks)   // ONE key switch over the n_out B extracted samples
        HIPCHK(launch_keyswitch(*f.key, j.n_out * j.B, u_a, u_b, nullptr, nullptr, 0, j.out_a, j.out_b, s));
    return TFHE_AMD_OK;
}

int lookup_dev(TfheAmdContext *c, TfheAmdTgsw *set, bool ks, int B, int d, const int32_t *sel, int n_tab, int n_poly,
               int tab_rows, const int32_t *tab, const int32_t *tab_index, int log_stride, int n_out, int32_t *out_a,
               int32_t *out_b, void *stream) {
    if (!c || !lookup_shape_ok(set, B, d, n_tab, n_poly, tab_rows, log_stride, n_out)) return TFHE_AMD_E_ARG;
    if (set->device != tfhe_amd_context_device(c) || set->count <= 0) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!tab || !out_a || !out_b || (d > 0 && !sel)) return TFHE_AMD_E_ARG;
    LookupJob j{set, ks, B, d, n_tab, n_poly, tab_rows, log_stride, n_out, sel, tab, tab_index, out_a, out_b};
    return tfhe_amd_internal_frame(c, stream, ks ? B * n_out : 0, lookup_in_frame, &j);
}

struct CmuxJob {
    TfheAmdTgsw *set;
    int B;
    const int32_t *sel, *d1, *d0;
    int32_t *out;
};

int cmux_in_frame(const ContextFrame &f, void *arg) {
    const CmuxJob &j = *static_cast<CmuxJob *>(arg);
    TgswCmux c;
    c.count = j.set->count;
    c.sel = j.sel;
    c.d0 = j.d0;
    c.d1 = j.d1;
    c.out = j.out;
    HIPCHK(launch_tgsw_cmux_v4(*f.key, j.set->v2, j.B, c, f.stream));
    return TFHE_AMD_OK;
}

struct HostLookupJob {
    TfheAmdContext *c;
    LookupJob j;   // host pointers
};

int lookup_host_in_frame(const ContextFrame &f, void *arg) {
    HostLookupJob &h = *static_cast<HostLookupJob *>(arg);
    const LookupJob &j = h.j;
    hipStream_t s = f.stream;
    const size_t n_sel = (size_t)j.B * j.d, n_tabw = (size_t)j.n_tab * j.n_poly * j.tab_rows * kN;
    const size_t n_res = (size_t)j.n_out * j.B, row = j.ks ? kn : kN;
    DevBufs bufs;
    int32_t *d_sel, *d_tab, *d_idx = nullptr, *d_a, *d_b;
    HIPCHK(bufs.get(&d_sel, n_sel));
    HIPCHK(bufs.get(&d_tab, n_tabw));
    if (j.tab_index) HIPCHK(bufs.get(&d_idx, (size_t)j.B));
    HIPCHK(bufs.get(&d_a, n_res * row));
    HIPCHK(bufs.get(&d_b, n_res));
    if (n_sel) HIPCHK(hipMemcpyAsync(d_sel, j.sel, sizeof(int32_t) * n_sel, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tab, j.tab, sizeof(int32_t) * n_tabw, hipMemcpyHostToDevice, s));
    if (j.tab_index) HIPCHK(hipMemcpyAsync(d_idx, j.tab_index, sizeof(int32_t) * j.B, hipMemcpyHostToDevice, s));
    hipError_t sync = hipSuccess;
    const int rc = lookup_dev(h.c, j.set, j.ks, j.B, j.d, d_sel, j.n_tab, j.n_poly, j.tab_rows, d_tab, d_idx,
                              j.log_stride, j.n_out, d_a, d_b, s);
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

int lookup_host(TfheAmdContext *c, TfheAmdTgsw *set, bool ks, int B, int d, const int32_t *sel, int n_tab, int n_poly,
                int tab_rows, const int32_t *tab, const int32_t *tab_index, int log_stride, int n_out, int32_t *out_a,
                int32_t *out_b) {
    if (!c || !lookup_shape_ok(set, B, d, n_tab, n_poly, tab_rows, log_stride, n_out)) return TFHE_AMD_E_ARG;
    if (set->device != tfhe_amd_context_device(c) || set->count <= 0) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!tab || !out_a || !out_b || (d > 0 && !sel)) return TFHE_AMD_E_ARG;
    for (size_t k = 0; k < (size_t)B * d; ++k)
        if (sel[k] < 0 || sel[k] >= set->count) return TFHE_AMD_E_ARG;
    if (tab_index)
        for (int q = 0; q < B; ++q)
            if (tab_index[q] < 0 || tab_index[q] >= n_tab) return TFHE_AMD_E_ARG;
    HostLookupJob h{c, {set, ks, B, d, n_tab, n_poly, tab_rows, log_stride, n_out, sel, tab, tab_index, out_a, out_b}};
    // the outer frame holds the context (the lock is recursive) from the uploads to the read-back
    return tfhe_amd_internal_frame(c, nullptr, 0, lookup_host_in_frame, &h);
}

}  // namespace

extern "C" int tfhe_amd_tgsw_import(TfheAmdContext *ctx, int n, const int32_t *coef_host, TfheAmdTgsw **out) {
    if (out) *out = nullptr;
    if (!ctx || !out || !coef_host || n <= 0 || n > (1 << 20)) return TFHE_AMD_E_ARG;
    TfheAmdTgsw *set = new TfheAmdTgsw();
    ImportJob j{n, coef_host, set};
    const int rc = tfhe_amd_internal_frame(ctx, nullptr, 0, import_in_frame, &j);
    if (rc != TFHE_AMD_OK) {
        if (set->v2) {
            DeviceScope dev_scope(tfhe_amd_context_device(ctx));
            (void)hipFree(set->v2);
        }
        delete set;
        return rc;
    }
    *out = set;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_tgsw_count(const TfheAmdTgsw *set) { return set ? set->count : TFHE_AMD_E_ARG; }

extern "C" int tfhe_amd_tgsw_destroy(TfheAmdTgsw *set) {
    if (!set) return TFHE_AMD_OK;
    {
        DeviceScope dev_scope(set->device);
        (void)hipDeviceSynchronize();   // launches on caller streams may still read the set
        set->fence.release();
        if (set->tree) (void)hipFree(set->tree);
        if (set->v2) (void)hipFree(set->v2);
    }
    delete set;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_tgsw_cmux_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, const int32_t *sel,
                                      const int32_t *d1, const int32_t *d0, int32_t *out, void *stream) {
    if (!ctx || !set || B < 0 || set->count <= 0 || set->device != tfhe_amd_context_device(ctx)) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!sel || !d1 || !out) return TFHE_AMD_E_ARG;
    CmuxJob j{set, B, sel, d1, d0, out};
    return tfhe_amd_internal_frame(ctx, stream, 0, cmux_in_frame, &j);
}

extern "C" int tfhe_amd_tgsw_lookup_woks_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, int d, const int32_t *sel,
                                             int n_tab, int n_poly, int tab_rows, const int32_t *tab,
                                             const int32_t *tab_index, int log_stride, int n_out, int32_t *u_a,
                                             int32_t *u_b, void *stream) {
    return lookup_dev(ctx, set, false, B, d, sel, n_tab, n_poly, tab_rows, tab, tab_index, log_stride, n_out, u_a, u_b,
                      stream);
}

extern "C" int tfhe_amd_tgsw_lookup_dev(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, int d, const int32_t *sel,
                                        int n_tab, int n_poly, int tab_rows, const int32_t *tab,
                                        const int32_t *tab_index, int log_stride, int n_out, int32_t *res_a,
                                        int32_t *res_b, void *stream) {
    return lookup_dev(ctx, set, true, B, d, sel, n_tab, n_poly, tab_rows, tab, tab_index, log_stride, n_out, res_a,
                      res_b, stream);
}

extern "C" int tfhe_amd_tgsw_lookup_woks_host(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, int d, const int32_t *sel,
                                              int n_tab, int n_poly, int tab_rows, const int32_t *tab,
                                              const int32_t *tab_index, int log_stride, int n_out, int32_t *u_a,
                                              int32_t *u_b) {
    return lookup_host(ctx, set, false, B, d, sel, n_tab, n_poly, tab_rows, tab, tab_index, log_stride, n_out, u_a, u_b);
}

extern "C" int tfhe_amd_tgsw_lookup_host(TfheAmdContext *ctx, TfheAmdTgsw *set, int B, int d, const int32_t *sel,
                                         int n_tab, int n_poly, int tab_rows, const int32_t *tab,
                                         const int32_t *tab_index, int log_stride, int n_out, int32_t *res_a,
                                         int32_t *res_b) {
    return lookup_host(ctx, set, true, B, d, sel, n_tab, n_poly, tab_rows, tab, tab_index, log_stride, n_out, res_a,
                       res_b);
}
