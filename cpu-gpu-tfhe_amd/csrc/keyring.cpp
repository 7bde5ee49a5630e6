// keyring.cpp — mixed-key batches of the batched C ABI (include/tfhe_amd.h): a ring
// of contexts on one device whose batch entry points take ciphertexts of any member's key in one
// call.  The batch is ordered by key slot (tfhe_amd_keyring_plan) into one table of rows; one blind
// rotation launch chain and one guard launch run all rows, each under its own bootstrapping key
// (k_blind_rotate_v6_rows_mk / k_blind_rotate_v4_rows_mk read the slot per row), and the unchanged
// key-switch launcher runs once per non-empty slot on that slot's slice of the table.  Inputs are
// read in place and results written in place through the rows' wire indices.
// The ring borrows its members' device keys and executes in member 0's frame, which it enters only
// through tfhe_amd_internal_frame (engine.h).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "api_internal.h"
#include "context.h"
#include "keyring_internal.h"

using namespace tfhe_amd;

namespace {

// blind rotations of one gate of the ring's gate forms: 2 (MUX), 1 (binary), 0 (NOT / COPY), -1 (refused)
int gate_rows(int gate) {
    int32_t k0, k1, k2;
    if (gate == TFHE_GATE_MUX) return 2;
    if (gate_spec(gate, &k0, &k1, &k2)) return 1;
    return gate == TFHE_GATE_NOT || gate == TFHE_GATE_COPY ? 0 : -1;
}

// counting sort of the batch by slot (stable); rows / nlin: blind rotations and linear entries
int plan(int B, int n_keys, const int *key_of, const int *gates, int *order, int *offsets, int *rows, int *nlin) {
    if (B < 0 || n_keys < 1 || n_keys > kRingMaxKeys || (B > 0 && !key_of)) return TFHE_AMD_E_ARG;
    int cnt[kRingMaxKeys + 1] = {0};
    long r = 0;
    int l = 0;
    for (int b = 0; b < B; ++b) {
        if (key_of[b] < 0 || key_of[b] >= n_keys) return TFHE_AMD_E_ARG;
        const int gr = gates ? gate_rows(gates[b]) : 1;
        if (gr < 0) return TFHE_AMD_E_ARG;
        r += gr;
        l += gr == 0;
        cnt[key_of[b] + 1]++;
    }
    if (r > 0x3fffffffL) return TFHE_AMD_E_ARG;
    for (int g = 0; g < n_keys; ++g) cnt[g + 1] += cnt[g];
    if (offsets) memcpy(offsets, cnt, sizeof(int) * (n_keys + 1));
    if (order)
        for (int b = 0; b < B; ++b) order[cnt[key_of[b]]++] = b;
    if (rows) *rows = (int)r;
    if (nlin) *nlin = l;
    return TFHE_AMD_OK;
}

struct RingJob {
    TfheAmdKeyRing *ring;
    int B;
    const int *gates, *key_of;   // host; gates null: the LUT form
    RingWires wires;             // device arrays
    RingLut lut;
    int32_t *res_a, *res_b;
    // the plan
    std::vector<int> order, offsets;
    int rows = 0, nlin = 0;
};

// the tables of one call in the ring's pinned block: [rows CircRow][nks CircKs][nlin CircLin][rows slot]
struct Tables {
    CircRow *rw;
    CircKs *ks;
    CircLin *lin;
    int32_t *row_key;
    size_t bytes;
    Tables(void *base, int rows, int nks, int nlin) {
        char *p = static_cast<char *>(base);
        rw = reinterpret_cast<CircRow *>(p);
        ks = reinterpret_cast<CircKs *>(p + sizeof(CircRow) * rows);
        lin = reinterpret_cast<CircLin *>(reinterpret_cast<char *>(ks) + sizeof(CircKs) * nks);
        row_key = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(lin) + sizeof(CircLin) * nlin);
        bytes = sizeof(CircRow) * rows + sizeof(CircKs) * nks + sizeof(CircLin) * nlin + sizeof(int32_t) * rows;
    }
};

int run_in_frame(const ContextFrame &f, void *arg) {
    RingJob &j = *static_cast<RingJob *>(arg);
    TfheAmdKeyRing *ring = j.ring;
    TfheAmdContext *c0 = ring->m[0];
    hipStream_t s = f.stream;
    const int n_keys = (int)ring->m.size(), B = j.B, nks = B - j.nlin;
    const size_t need = Tables(nullptr, j.rows, nks, j.nlin).bytes;
    if (need > ring->tab_bytes) {
        HIPCHK(hipDeviceSynchronize());   // the tables may still be in use on another stream
        if (ring->h_tab) (void)hipHostFree(ring->h_tab);
        if (ring->d_tab) (void)hipFree(ring->d_tab);
        ring->h_tab = ring->d_tab = nullptr;
        ring->tab_bytes = 0;
        size_t cap = 4096;
        while (cap < need) cap *= 2;
        HIPCHK(hipHostMalloc(&ring->h_tab, cap, hipHostMallocDefault));
        HIPCHK(hipMalloc(&ring->d_tab, cap));
        ring->tab_bytes = cap;
    }
    if (!ring->up) HIPCHK(hipEventCreateWithFlags(&ring->up, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(ring->up));   // the previous call's upload has left the pinned block
    Tables h(ring->h_tab, j.rows, nks, j.nlin), d(ring->d_tab, j.rows, nks, j.nlin);
    std::vector<int> ks_off(n_keys + 1, 0);
    int r = 0, k = 0, l = 0;
    for (int g = 0; g < n_keys; ++g) {
        ks_off[g] = k;
        for (int p = j.offsets[g]; p < j.offsets[g + 1]; ++p) {
            const int b = j.order[p];
            const int gate = j.gates ? j.gates[b] : -1;
            if (!j.gates) {   // LUT form: x alone, its table picked by the kernel from lut_index[b]
                h.rw[r] = CircRow{0, 1, 0, 0, 4 * b, -1, -1, 0};
                h.row_key[r] = g;
                h.ks[k++] = CircKs{r, -1, 0, b};
                r += 1;
            } else if (gate == TFHE_GATE_MUX) {   // boot-gates.cu:407-448, as tfhe_amd_gate_batch_mixed_host
                h.rw[r] = CircRow{-kMu, 1, 1, 0, 4 * b, 4 * b + 1, -1, 0};
                h.rw[r + 1] = CircRow{-kMu, -1, 1, 0, 4 * b, 4 * b + 2, -1, 0};
                h.row_key[r] = h.row_key[r + 1] = g;
                h.ks[k++] = CircKs{r, r + 1, kMu, b};
                r += 2;
            } else if (gate == TFHE_GATE_NOT || gate == TFHE_GATE_COPY) {
                h.lin[l++] = CircLin{0, gate == TFHE_GATE_NOT ? -1 : 1, 4 * b, b};
            } else {
                int32_t k0, k1, k2;
                gate_spec(gate, &k0, &k1, &k2);
                h.rw[r] = CircRow{k0, k1, k2, 0, 4 * b, 4 * b + 1, -1, 0};
                h.row_key[r] = g;
                h.ks[k++] = CircKs{r, -1, 0, b};
                r += 1;
            }
        }
    }
    ks_off[n_keys] = k;
    HIPCHK(ring->fence.acquire(s));
    HIPCHK(hipMemcpyAsync(ring->d_tab, ring->h_tab, h.bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ring->up, s));
    if (j.rows > 0) {
        ProfScope ps(c0, s, true);
        const BrMode mode = j.gates ? BrMode::Const : BrMode::Lut;
        const Guard gd = ctx_guard(c0);
        const RingKeys k6{ring->d_fft, d.row_key, n_keys}, k4{ring->d_v2, d.row_key, n_keys};
        if (br_version() == 4) {
            HIPCHK(launch_blind_rotate_v4_rows_ring(*f.key, k4, j.rows, d.rw, j.wires, j.lut, kMu, f.u_a, f.u_b, s, mode));
        } else {
            HIPCHK(launch_blind_rotate_v6_rows_ring(*f.key, k6, j.rows, d.rw, j.wires, j.lut, kMu, f.u_a, f.u_b, s, mode,
                                                    &gd));
            if (gd.flags)
                HIPCHK(launch_blind_rotate_v4_rows_ring(*f.key, k4, j.rows, d.rw, j.wires, j.lut, kMu, f.u_a, f.u_b, s,
                                                        mode, &gd));
        }
    }
    {
        ProfScope ps(c0, s, false);
        for (int g = 0; g < n_keys; ++g) {
            const int n = ks_off[g + 1] - ks_off[g];
            if (n <= 0) continue;
            char label[48];
            snprintf(label, sizeof label, "keyring_keyswitch(slot=%d+n=%d)", g, n);
            trace_kernel(label);
            HIPCHK(launch_keyswitch_rows(ring->m[g]->key, 1, n, d.ks + ks_off[g], f.u_a, f.u_b, j.res_a, j.res_b, s));
        }
    }
    HIPCHK(launch_ring_linear(j.nlin, d.lin, j.wires, j.res_a, j.res_b, s));
    HIPCHK(ring->fence.done(s));
    return TFHE_AMD_OK;
}

// argument rules of both forms (no array is read but the two host ones); 1: nothing to do
int ring_args(TfheAmdKeyRing *ring, RingJob &j) {
    if (!ring || j.B < 0) return TFHE_AMD_E_ARG;
    if (j.B == 0) return 1;
    const int n_keys = (int)ring->m.size();
    j.order.resize(j.B);
    j.offsets.resize(n_keys + 1);
    const int rc = plan(j.B, n_keys, j.key_of, j.gates, j.order.data(), j.offsets.data(), &j.rows, &j.nlin);
    if (rc) return rc;
    if (!j.res_a || !j.res_b || !j.wires.a0 || !j.wires.b0) return TFHE_AMD_E_ARG;
    if (j.gates) {
        bool binary = false, mux = false;
        for (int b = 0; b < j.B; ++b) {
            const int gr = gate_rows(j.gates[b]);
            binary |= gr >= 1;
            mux |= gr == 2;
        }
        if (binary && (!j.wires.a1 || !j.wires.b1)) return TFHE_AMD_E_ARG;
        if (mux && (!j.wires.a2 || !j.wires.b2)) return TFHE_AMD_E_ARG;
    } else if (!j.lut.tv || j.lut.n_lut < 1) {
        return TFHE_AMD_E_ARG;
    }
    return TFHE_AMD_OK;
}

// caller holds ring->mu
int run_locked(RingJob &j, void *stream) {
    // u scratch and guard flags for `rows` rows: a context slot holds two of each (the MUX's halves)
    return tfhe_amd_internal_frame(j.ring->m[0], stream, (j.rows + 1) / 2, run_in_frame, &j);
}

int run_dev(RingJob &j, void *stream) {
    const int rc = ring_args(j.ring, j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    std::lock_guard<std::mutex> lock(j.ring->mu);
    return run_locked(j, stream);
}

// temporary device buffers of the host forms, freed on every path
struct DevBufs {
    std::vector<void *> p;
    ~DevBufs() {
        for (void *q : p) (void)hipFree(q);
    }
    hipError_t get(int32_t **out, size_t words) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, sizeof(int32_t) * (words ? words : 1));
        if (e == hipSuccess) p.push_back(q);
        *out = static_cast<int32_t *>(q);
        return e;
    }
};

// The host forms: the job's arrays are host arrays; they are staged into device buffers on member
// 0's stream, run through the device path and read back, synchronously.  extra: further host input
// blocks (pointer, words, where the device pointer goes), the LUT form's tables and indices.
struct HostBlock {
    const int32_t *h;
    size_t words;
    const int32_t **d;
};
int run_host(RingJob &j, std::vector<HostBlock> in) {
    const int rc = ring_args(j.ring, j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    TfheAmdKeyRing *ring = j.ring;
    std::lock_guard<std::mutex> lock(ring->mu);
    DeviceScope dev_scope(ring->device);
    HIPCHK(dev_scope.rc);
    hipStream_t s = (hipStream_t)tfhe_amd_context_stream(ring->m[0]);
    const size_t B = (size_t)j.B;
    DevBufs bufs;
    for (HostBlock &b : in) {
        if (!b.h) continue;
        int32_t *d;
        HIPCHK(bufs.get(&d, b.words));
        HIPCHK(hipMemcpyAsync(d, b.h, sizeof(int32_t) * b.words, hipMemcpyHostToDevice, s));
        *b.d = d;
    }
    int32_t *h_a = j.res_a, *h_b = j.res_b;
    HIPCHK(bufs.get(&j.res_a, B * kn));
    HIPCHK(bufs.get(&j.res_b, B));
    const int run = run_locked(j, s);
    hipError_t e = hipSuccess;
    if (run == TFHE_AMD_OK) e = hipMemcpyAsync(h_a, j.res_a, sizeof(int32_t) * B * kn, hipMemcpyDeviceToHost, s);
    if (run == TFHE_AMD_OK && e == hipSuccess) e = hipMemcpyAsync(h_b, j.res_b, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s);
    const hipError_t sync = hipStreamSynchronize(s);   // before the buffers go, whatever happened
    if (run != TFHE_AMD_OK) return run;
    HIPCHK(e);
    HIPCHK(sync);
    return TFHE_AMD_OK;
}

}  // namespace

extern "C" int tfhe_amd_keyring_plan(int B, int n_keys, const int *key_of, const int *gates, int *order, int *offsets,
                                     int *rows) {
    return plan(B, n_keys, key_of, gates, order, offsets, rows, nullptr);
}

extern "C" int tfhe_amd_keyring_create(TfheAmdContext *const *ctxs, int n_keys, TfheAmdKeyRing **out) {
    if (out) *out = nullptr;
    if (!ctxs || !out || n_keys < 1 || n_keys > kRingMaxKeys) return TFHE_AMD_E_ARG;
    for (int g = 0; g < n_keys; ++g) {
        const TfheAmdContext *c = ctxs[g];
        if (!c || c->device != ctxs[0]->device) return TFHE_AMD_E_ARG;
        const DeviceKey &k = c->key;
        if (!k.has_bk || !k.bk_fft || !k.bk_v2 || !k.ksk || !(k.ksk4 || k.ksk5)) return TFHE_AMD_E_ARG;
    }
    TfheAmdKeyRing *ring = new TfheAmdKeyRing();
    ring->m.assign(ctxs, ctxs + n_keys);
    ring->device = ctxs[0]->device;
    std::vector<void *> fft(n_keys), v2(n_keys);
    for (int g = 0; g < n_keys; ++g) {
        fft[g] = ctxs[g]->key.bk_fft;
        v2[g] = ctxs[g]->key.bk_v2;
    }
    DeviceScope dev_scope(ring->device);
    const size_t bytes = sizeof(void *) * n_keys;
    if (dev_scope.rc != hipSuccess || hipMalloc(&ring->d_fft, bytes) != hipSuccess ||
        hipMalloc(&ring->d_v2, bytes) != hipSuccess ||
        hipMemcpy(ring->d_fft, fft.data(), bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ring->d_v2, v2.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        tfhe_amd_keyring_destroy(ring);
        return TFHE_AMD_E_HIP;
    }
    *out = ring;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_keyring_destroy(TfheAmdKeyRing *ring) {
    if (!ring) return TFHE_AMD_OK;
    tfhe_amd_internal_circuits_forget_context(ring->uid);   // circuits' device state of runs on this ring
    {
        DeviceScope dev_scope(ring->device);
        (void)hipDeviceSynchronize();   // launches on caller streams may still read the tables
        ring->fence.release();
        if (ring->up) (void)hipEventDestroy(ring->up);
        if (ring->h_tab) (void)hipHostFree(ring->h_tab);
        if (ring->d_tab) (void)hipFree(ring->d_tab);
        if (ring->d_fft) (void)hipFree(ring->d_fft);
        if (ring->d_v2) (void)hipFree(ring->d_v2);
    }
    delete ring;
    return TFHE_AMD_OK;
}

extern "C" int tfhe_amd_keyring_count(const TfheAmdKeyRing *ring) {
    return ring ? (int)ring->m.size() : TFHE_AMD_E_ARG;
}
extern "C" int tfhe_amd_keyring_device(const TfheAmdKeyRing *ring) { return ring ? ring->device : -1; }

extern "C" int tfhe_amd_keyring_gate_batch_dev(TfheAmdKeyRing *ring, int B, const int *gates, const int *key_of,
                                               int32_t *res_a, int32_t *res_b, const int32_t *ca_a,
                                               const int32_t *ca_b, const int32_t *cb_a, const int32_t *cb_b,
                                               const int32_t *cc_a, const int32_t *cc_b, void *stream) {
    if (B > 0 && !gates) return TFHE_AMD_E_ARG;
    RingJob j{ring, B, gates, key_of, RingWires{ca_a, ca_b, cb_a, cb_b, cc_a, cc_b, B}, RingLut{}, res_a, res_b};
    return run_dev(j, stream);
}

extern "C" int tfhe_amd_keyring_gate_batch_host(TfheAmdKeyRing *ring, int B, const int *gates, const int *key_of,
                                                int32_t *res_a, int32_t *res_b, const int32_t *ca_a,
                                                const int32_t *ca_b, const int32_t *cb_a, const int32_t *cb_b,
                                                const int32_t *cc_a, const int32_t *cc_b) {
    if (B > 0 && !gates) return TFHE_AMD_E_ARG;
    RingJob j{ring, B, gates, key_of, RingWires{ca_a, ca_b, cb_a, cb_b, cc_a, cc_b, B}, RingLut{}, res_a, res_b};
    const size_t n = B > 0 ? (size_t)B : 0;
    RingWires &w = j.wires;
    return run_host(j, {{ca_a, n * kn, &w.a0}, {ca_b, n, &w.b0}, {cb_a, n * kn, &w.a1}, {cb_b, n, &w.b1},
                        {cc_a, n * kn, &w.a2}, {cc_b, n, &w.b2}});
}

extern "C" int tfhe_amd_keyring_bootstrap_lut_batch_dev(TfheAmdKeyRing *ring, int B, const int *key_of, int n_lut,
                                                        const int32_t *tv, const int32_t *lut_index, int32_t *res_a,
                                                        int32_t *res_b, const int32_t *x_a, const int32_t *x_b,
                                                        void *stream) {
    if (n_lut < 1 || !tv) return TFHE_AMD_E_ARG;
    RingJob j{ring, B, nullptr, key_of, RingWires{x_a, x_b, nullptr, nullptr, nullptr, nullptr, B},
              RingLut{tv, lut_index, n_lut}, res_a, res_b};
    return run_dev(j, stream);
}

extern "C" int tfhe_amd_keyring_bootstrap_lut_batch_host(TfheAmdKeyRing *ring, int B, const int *key_of, int n_lut,
                                                         const int32_t *tv, const int32_t *lut_index, int32_t *res_a,
                                                         int32_t *res_b, const int32_t *x_a, const int32_t *x_b) {
    if (n_lut < 1 || !tv) return TFHE_AMD_E_ARG;
    RingJob j{ring, B, nullptr, key_of, RingWires{x_a, x_b, nullptr, nullptr, nullptr, nullptr, B},
              RingLut{tv, lut_index, n_lut}, res_a, res_b};
    const size_t n = B > 0 ? (size_t)B : 0;
    return run_host(j, {{x_a, n * kn, &j.wires.a0}, {x_b, n, &j.wires.b0}, {tv, (size_t)n_lut * kN, &j.lut.tv},
                        {lut_index, n, &j.lut.lut_index}});
}
