// circuit_select.cpp — the select part of a circuit run: per level with select rows,
// the pack of every row's candidates out of the wire table, the box fill per group of equal p and the
// rows launch of the blind rotation that starts from those samples; and the run form that carries the
// pack key, tfhe_amd_circuit_run_pk_dev.  The circuit compiler and runner (circuit.cpp) reach this
// file only through the per-level hook of circuit_internal.h, so they name none of these launchers
// and still build against the stand-in kernels of the ThreadSanitizer tests.  The accumulator and
// digit scratch stay with the pack key, grown under its lock and fenced like the selection calls'
// (acc.cpp select_in_frame).
#include <mutex>

#include "circuit_internal.h"
#include "context.h"
#include "pack_key.h"

using namespace tfhe_amd;

namespace tfhe_amd {

// The rows launch of a level's select rows with the selected kernel, as launch_blind_rotate_rows does
// for the other modes: the fp64 kernel guarded (then the exact kernel over the flags it wrote), or the
// exact kernel alone under tfhe_amd_select_kernel(4).
hipError_t launch_blind_rotate_rows_tlwe(const DeviceKey &key, int B, int nrows, const CircRow *rows, const int32_t *wa,
                                         const int32_t *wb, const int32_t *acc, int32_t *u_a, int32_t *u_b,
                                         hipStream_t s, const Guard *guard) {
    if (br_version() == 4) return launch_blind_rotate_v4_rows_tlwe(key, B, nrows, rows, wa, wb, acc, u_a, u_b, s);
    const hipError_t e = launch_blind_rotate_v6_rows_tlwe(key, B, nrows, rows, wa, wb, acc, u_a, u_b, s, guard);
    if (e != hipSuccess || !guard || !guard->flags) return e;
    return launch_blind_rotate_v4_rows_tlwe(key, B, nrows, rows, wa, wb, acc, u_a, u_b, s, guard);
}

}  // namespace tfhe_amd

namespace {

constexpr size_t kDigWords = (size_t)kn * kN;   // digit scratch of one output (pack.cpp)
constexpr size_t kAccWords = (size_t)2 * kN;    // one TLWE sample

int log2_of(int p) {
    int l = 0;
    while ((1 << l) < p) ++l;
    return l;
}

// One level's select rows: output t = r B + k of the pack is the accumulator of row r at instance k.
int select_level(void *arg, const DeviceKey &dkey, const CircSelLevel &lv, hipStream_t s) {
    TfheAmdPackKey *key = static_cast<TfheAmdPackKey *>(arg);
    const long total = (long)lv.nsel * lv.B;
    if (total <= 0) return TFHE_AMD_OK;
    if (total > 0x3fffffffL) return TFHE_AMD_E_ARG;
    std::lock_guard<std::mutex> lock(key->mu);
    const size_t need_dig = (size_t)(total < kPackMaxBatch ? total : kPackMaxBatch), need_acc = (size_t)total;
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
    for (long t0 = 0; t0 < total; t0 += kPackMaxBatch) {   // batches share the digit scratch in stream order
        const int Tc = (int)(total - t0 < kPackMaxBatch ? total - t0 : kPackMaxBatch);
        HIPCHK(launch_pack_rows(dkey, key->v2, Tc, (int)t0, lv.B, lv.n_wires, lv.d_sel, lv.wa, lv.wb, key->dig,
                                pack_split(Tc, key->cus), key->acc + (size_t)t0 * kAccWords, s));
    }
    for (int r0 = 0; r0 < lv.nsel;) {   // one box fill per group of equal p (the rows are grouped by p)
        int r1 = r0 + 1;
        while (r1 < lv.nsel && lv.h_sel[r1].p == lv.h_sel[r0].p) ++r1;
        int32_t *grp = key->acc + (size_t)r0 * lv.B * kAccWords;
        HIPCHK(launch_tlwe_box_fill((r1 - r0) * lv.B, kLogN - log2_of(lv.h_sel[r0].p), grp, grp, s));
        r0 = r1;
    }
    const hipError_t e = launch_blind_rotate_rows_tlwe(dkey, lv.B, lv.nsel, lv.d_rows, lv.wa, lv.wb, key->acc, lv.u_a,
                                                       lv.u_b, s, &lv.guard);
    HIPCHK(key->fence.done(s));   // whatever was enqueued is ordered before the scratch's next user
    HIPCHK(e);
    return TFHE_AMD_OK;
}

}  // namespace

extern "C" int tfhe_amd_circuit_run_pk_dev(TfheAmdContext *c, TfheAmdPackKey *pack_key, TfheAmdCircuit *circ, int B,
                                           int32_t *wires_a, int32_t *wires_b, void *stream) {
    if (!c || !circ || !pack_key || !pack_key->v2 || B < 0 || !c->key.has_bk || !(c->key.ksk4 || c->key.ksk5))
        return TFHE_AMD_E_ARG;
    if (pack_key->device != c->device) return TFHE_AMD_E_ARG;
    if (B == 0) return TFHE_AMD_OK;
    if (!wires_a || !wires_b) return TFHE_AMD_E_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    EntryFrame frame(c, 0);
    if (frame.rc) return frame.rc;
    const CircSelectHook hook{select_level, pack_key};
    return tfhe_amd_circuit_run_dev_hook(c->uid, c->key, c->device, s, circ, B, wires_a, wires_b, c->gstats, &hook);
}
