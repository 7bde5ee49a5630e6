// keyring_circuit.cpp — mixed-key circuits (include/tfhe_amd.h): one run of a circuit
// over B instances, instance k under the cloud key of ring slot key_of[k].  The circuit runner
// (circuit.cpp) keeps its schedule, its level tables, its u scratch (keyed by the ring's own id) and
// the key-independent linear launch; through the level hook of circuit_internal.h it hands each
// bootstrapped level to this file, which enqueues
//   * one blind-rotation launch chain and one guard launch over all rows x instances, each instance
//     under its own bootstrapping key (k_blind_rotate_v6_rows_mkc / k_blind_rotate_v4_rows_mkc), and
//   * one key-switch launch over all key groups (k_keyswitch_v5 with the tiled lane map), or, where
//     that form does not apply, one launch of the single-key kernels per non-empty group.
// The run executes in member 0's frame, entered only through tfhe_amd_internal_frame, under the
// ring's lock; the call's tables go through the ring's pinned block like a gate batch's (keyring.cpp).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "api_internal.h"
#include "circuit_internal.h"
#include "context.h"
#include "keyring_internal.h"

using namespace tfhe_amd;

namespace {

// counting sort of the instances by slot (stable), then the M-tiles of each group's nks n_g lanes;
// tiles null: counted only
int plan(int B, int n_keys, const int *key_of, int nks, int tile, int *order, int *offsets, int *tiles, int tile_cap,
         int *n_tiles) {
    if (B < 0 || n_keys < 1 || n_keys > kRingMaxKeys || nks < 0 || tile < 1 || (B > 0 && !key_of))
        return TFHE_AMD_E_ARG;
    if ((long)B * nks > 0x3fffffffL) return TFHE_AMD_E_ARG;
    int cnt[kRingMaxKeys + 1] = {0};
    for (int k = 0; k < B; ++k) {
        if (key_of[k] < 0 || key_of[k] >= n_keys) return TFHE_AMD_E_ARG;
        cnt[key_of[k] + 1]++;
    }
    for (int g = 0; g < n_keys; ++g) cnt[g + 1] += cnt[g];
    int nt = 0;
    for (int g = 0; g < n_keys; ++g) {
        const int lanes = nks * (cnt[g + 1] - cnt[g]), base = nks * cnt[g];
        for (int l0 = 0; l0 < lanes; l0 += tile, ++nt) {
            if (!tiles) continue;
            if (nt >= tile_cap) return TFHE_AMD_E_ARG;
            tiles[3 * nt] = g;
            tiles[3 * nt + 1] = base + l0;
            tiles[3 * nt + 2] = std::min(tile, lanes - l0);
        }
    }
    if (n_tiles) *n_tiles = nt;
    if (offsets) memcpy(offsets, cnt, sizeof(int) * (n_keys + 1));
    if (order)
        for (int k = 0; k < B; ++k) order[cnt[key_of[k]]++] = k;
    return TFHE_AMD_OK;
}

struct RingCircJob {
    TfheAmdKeyRing *ring;
    TfheAmdCircuit *circ;
    int B;
    const int *key_of;         // host
    int32_t *wa, *wb;          // device wire table
    // the plan
    std::vector<int> order, offsets;
    std::vector<int> level_nks;               // per circuit level (0: nothing key-switched)
    std::map<int, std::vector<int>> tiles;    // nks -> tile records (slot, first, live)
    uint64_t schedule = 0;                    // the circuit's schedule the plan was made against
    int groups = 0;                           // non-empty key groups
    bool tiled = false;                       // the one-launch key switch applies
    // device side of the call's tables, set in the frame
    const int64_t *d_ksk5_off = nullptr;
    const int32_t *d_inst_key = nullptr, *d_order = nullptr, *d_offsets = nullptr;
    std::map<int, const KsTile *> d_tiles;    // nks -> its tile table
};

// the call's tables in the ring's block: [n_keys ksk5 distances][B inst_key][B order][n_keys + 1 offsets]
// then the tile tables of the distinct nks in ascending order
size_t tables_bytes(const RingCircJob &j, int n_keys) {
    size_t b = sizeof(int64_t) * n_keys + sizeof(int32_t) * (2 * (size_t)j.B + n_keys + 1);
    for (const auto &t : j.tiles) b += sizeof(int32_t) * t.second.size();
    return b;
}

// one bootstrapped level (circuit_internal.h CircLevelHook)
int ring_level(void *arg, const CircLevelJob &lv, hipStream_t s) {
    RingCircJob &j = *static_cast<RingCircJob *>(arg);
    TfheAmdKeyRing *ring = j.ring;
    TfheAmdContext *c0 = ring->m[0];
    const int n_keys = (int)ring->m.size();
    {
        ProfScope ps(c0, s, true);
        const RingInstKeys k6{ring->d_fft, j.d_inst_key, n_keys}, k4{ring->d_v2, j.d_inst_key, n_keys};
        if (br_version() == 4) {
            HIPCHK(launch_blind_rotate_v4_rows_ringc(c0->key, k4, lv.B, lv.nrows, lv.d_rows, lv.wa, lv.wb, kMu, lv.u_a,
                                                     lv.u_b, s, lv.mode));
        } else {
            HIPCHK(launch_blind_rotate_v6_rows_ringc(c0->key, k6, lv.B, lv.nrows, lv.d_rows, lv.wa, lv.wb, kMu, lv.u_a,
                                                     lv.u_b, s, lv.mode, &lv.guard));
            if (lv.guard.flags)
                HIPCHK(launch_blind_rotate_v4_rows_ringc(c0->key, k4, lv.B, lv.nrows, lv.d_rows, lv.wa, lv.wb, kMu,
                                                         lv.u_a, lv.u_b, s, lv.mode, &lv.guard));
        }
    }
    if (lv.nks <= 0) return TFHE_AMD_OK;
    ProfScope ps(c0, s, false);
    char label[80];   // the launch trace keeps a name once: the label tells the levels' launches apart
    if (j.tiled) {
        const auto it = j.d_tiles.find(lv.nks);
        if (it == j.d_tiles.end()) return TFHE_AMD_E_ARG;   // (not reached: the runner checked the schedule)
        const RingKsTiles t{ring->m[0]->key.ksk5, j.d_ksk5_off, j.d_order, j.d_offsets, it->second, n_keys,
                            (int)(j.tiles[lv.nks].size() / 3)};
        snprintf(label, sizeof label, "keyring_circuit_keyswitch(level=%d+tiles=%d)", lv.level, t.ntiles);
        trace_kernel(label);
        HIPCHK(launch_keyswitch_rows_tiles(t, lv.B, lv.nks, lv.d_ks, lv.u_a, lv.u_b, lv.wa, lv.wb, s));
        return TFHE_AMD_OK;
    }
    for (int g = 0; g < n_keys; ++g) {
        const int n = j.offsets[g + 1] - j.offsets[g];
        if (n <= 0) continue;
        snprintf(label, sizeof label, "keyring_circuit_keyswitch(level=%d+slot=%d+n=%d)", lv.level, g, n);
        trace_kernel(label);
        HIPCHK(launch_keyswitch_rows_inst(ring->m[g]->key, lv.B, lv.nks, lv.d_ks, j.d_order + j.offsets[g], n, lv.u_a,
                                          lv.u_b, lv.wa, lv.wb, s));
    }
    return TFHE_AMD_OK;
}

int run_in_frame(const ContextFrame &f, void *arg) {
    RingCircJob &j = *static_cast<RingCircJob *>(arg);
    TfheAmdKeyRing *ring = j.ring;
    TfheAmdContext *c0 = ring->m[0];
    hipStream_t s = f.stream;
    const int n_keys = (int)ring->m.size(), B = j.B;
    const size_t need = tables_bytes(j, n_keys);
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
    {
        char *h = static_cast<char *>(ring->h_tab), *d = static_cast<char *>(ring->d_tab);
        size_t off = 0;
        // each member's ksk5 as its distance from member 0's in 16-byte units (engine.h RingKsTiles)
        int64_t *kd = reinterpret_cast<int64_t *>(h);
        const intptr_t base5 = reinterpret_cast<intptr_t>(ring->m[0]->key.ksk5);
        for (int g = 0; g < n_keys; ++g) kd[g] = (reinterpret_cast<intptr_t>(ring->m[g]->key.ksk5) - base5) / 16;
        j.d_ksk5_off = reinterpret_cast<const int64_t *>(d);
        off += sizeof(int64_t) * n_keys;
        int32_t *ik = reinterpret_cast<int32_t *>(h + off);
        for (int k = 0; k < B; ++k) ik[k] = j.key_of[k];
        j.d_inst_key = reinterpret_cast<const int32_t *>(d + off);
        off += sizeof(int32_t) * B;
        memcpy(h + off, j.order.data(), sizeof(int32_t) * B);
        j.d_order = reinterpret_cast<const int32_t *>(d + off);
        off += sizeof(int32_t) * B;
        memcpy(h + off, j.offsets.data(), sizeof(int32_t) * (n_keys + 1));
        j.d_offsets = reinterpret_cast<const int32_t *>(d + off);
        off += sizeof(int32_t) * (n_keys + 1);
        for (const auto &t : j.tiles) {
            static_assert(sizeof(KsTile) == 3 * sizeof(int32_t), "a tile record is three words");
            memcpy(h + off, t.second.data(), sizeof(int32_t) * t.second.size());
            j.d_tiles[t.first] = reinterpret_cast<const KsTile *>(d + off);
            off += sizeof(int32_t) * t.second.size();
        }
    }
    HIPCHK(ring->fence.acquire(s));
    HIPCHK(hipMemcpyAsync(ring->d_tab, ring->h_tab, need, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ring->up, s));
    const CircLevelHook hook{ring_level, &j, j.schedule};
    const int rc = tfhe_amd_circuit_run_dev_hooks(ring->uid, c0->key, ring->device, s, j.circ, B, j.wa, j.wb, c0->gstats,
                                                  nullptr, &hook);
    HIPCHK(ring->fence.done(s));   // whatever was enqueued is ordered before the tables' next user
    return rc;
}

// argument rules of both forms and the plan (nothing is launched or written); 1: nothing to do
int ring_args(RingCircJob &j) {
    TfheAmdKeyRing *ring = j.ring;
    if (!ring || !j.circ || !j.key_of || j.B < 0) return TFHE_AMD_E_ARG;
    const int n_keys = (int)ring->m.size(), B = j.B;
    for (int k = 0; k < B; ++k)
        if (j.key_of[k] < 0 || j.key_of[k] >= n_keys) return TFHE_AMD_E_ARG;
    int has_select = 0;
    int rc = tfhe_amd_internal_circuit_levels(j.circ, &j.level_nks, &has_select, &j.schedule);
    if (rc) return rc;
    if (has_select) return TFHE_AMD_E_ARG;   // packing keys are per key
    if (B == 0) return 1;
    if (!j.wa || !j.wb) return TFHE_AMD_E_ARG;
    j.order.resize(B);
    j.offsets.resize(n_keys + 1);
    rc = plan(B, n_keys, j.key_of, 0, 1, j.order.data(), j.offsets.data(), nullptr, 0, nullptr);
    if (rc) return rc;
    bool all_ks5 = true;
    for (int g = 0; g < n_keys; ++g) {
        j.groups += j.offsets[g + 1] > j.offsets[g];
        all_ks5 = all_ks5 && ring->m[g]->key.ksk5;
    }
#ifdef TFHE_AMD_RING_KS_PER_GROUP   // variant builds: the per-group key switch everywhere
    all_ks5 = false;
#endif
    // one launch over all groups when every member has the int8 key layout and the level's lanes lie
    // in more than one group (every group has the same outputs, so that holds for all levels or none)
    j.tiled = all_ks5 && j.groups > 1;
    if (!j.tiled) return TFHE_AMD_OK;
    const int tile = ks5_tile_lanes();
    for (int nks : j.level_nks) {
        if (nks <= 0 || j.tiles.count(nks)) continue;
        // one pass: a group's last tile may be partial, so at most groups + nks B / tile tiles
        if ((long)nks * B > 0x3fffffffL) return TFHE_AMD_E_ARG;
        int nt = 0;
        const int cap = j.groups + (int)((long)nks * B / tile);
        std::vector<int> &t = j.tiles[nks];
        t.resize(3 * (size_t)cap);
        rc = plan(B, n_keys, j.key_of, nks, tile, nullptr, nullptr, t.data(), cap, &nt);
        if (rc) return rc;
        t.resize(3 * (size_t)nt);
    }
    return TFHE_AMD_OK;
}

// caller holds ring->mu
int run_locked(RingCircJob &j, void *stream) {
    return tfhe_amd_internal_frame(j.ring->m[0], stream, 0, run_in_frame, &j);
}

}  // namespace

extern "C" int tfhe_amd_keyring_circuit_plan(int B, int n_keys, const int *key_of, int nks, int tile, int *order,
                                             int *offsets, int *tiles, int tile_cap, int *n_tiles) {
    return plan(B, n_keys, key_of, nks, tile, order, offsets, tiles, tiles ? tile_cap : 0, n_tiles);
}

extern "C" int tfhe_amd_keyring_circuit_tile(void) { return ks5_tile_lanes(); }

extern "C" int tfhe_amd_keyring_circuit_run_dev(TfheAmdKeyRing *ring, TfheAmdCircuit *circ, int B, const int *key_of,
                                                int32_t *wires_a, int32_t *wires_b, void *stream) {
    RingCircJob j{ring, circ, B, key_of, wires_a, wires_b};
    const int rc = ring_args(j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    std::lock_guard<std::mutex> lock(ring->mu);
    return run_locked(j, stream);
}

extern "C" int tfhe_amd_keyring_circuit_run_host(TfheAmdKeyRing *ring, TfheAmdCircuit *circ, int B, const int *key_of,
                                                 int n_in, const int *in_wires, const int32_t *in_a,
                                                 const int32_t *in_b, int n_out, const int *out_wires, int32_t *out_a,
                                                 int32_t *out_b) {
    if (!ring || !circ || !key_of || B < 0 || n_in < 0 || n_out < 0) return TFHE_AMD_E_ARG;
    if ((n_in && B && (!in_wires || !in_a || !in_b)) || (n_out && B && (!out_wires || !out_a || !out_b)))
        return TFHE_AMD_E_ARG;
    int n_wires = 0;
    int rc = tfhe_amd_circuit_info(circ, &n_wires, nullptr, nullptr, nullptr);
    if (rc != TFHE_AMD_OK) return rc;
    if (B > 0) {
        for (int k = 0; k < n_in; ++k)
            if (in_wires[k] < 0 || in_wires[k] >= n_wires) return TFHE_AMD_E_ARG;
        for (int k = 0; k < n_out; ++k)
            if (out_wires[k] < 0 || out_wires[k] >= n_wires) return TFHE_AMD_E_ARG;
    }
    int32_t dummy = 0;   // the argument rules see a wire table; the real one is allocated below
    RingCircJob j{ring, circ, B, key_of, &dummy, &dummy};
    rc = ring_args(j);
    if (rc != TFHE_AMD_OK) return rc == 1 ? TFHE_AMD_OK : rc;
    std::lock_guard<std::mutex> lock(ring->mu);
    DeviceScope dev_scope(ring->device);
    HIPCHK(dev_scope.rc);
    hipStream_t s = (hipStream_t)tfhe_amd_context_stream(ring->m[0]);
    const size_t nb = (size_t)B;
    int32_t *wa = nullptr, *wb = nullptr;
    if (hipMalloc(&wa, sizeof(int32_t) * (size_t)n_wires * nb * kn) != hipSuccess) return TFHE_AMD_E_NOMEM;
    if (hipMalloc(&wb, sizeof(int32_t) * (size_t)n_wires * nb) != hipSuccess) {
        (void)hipFree(wa);
        return TFHE_AMD_E_NOMEM;
    }
    hipError_t e = hipSuccess;
    for (int k = 0; k < n_in && e == hipSuccess; ++k) {   // a wire's plane [B][500] is contiguous on both sides
        e = hipMemcpyAsync(wa + (size_t)in_wires[k] * nb * kn, in_a + (size_t)k * nb * kn, sizeof(int32_t) * nb * kn,
                           hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(wb + (size_t)in_wires[k] * nb, in_b + (size_t)k * nb, sizeof(int32_t) * nb,
                               hipMemcpyHostToDevice, s);
    }
    j.wa = wa;
    j.wb = wb;
    const int run = e == hipSuccess ? run_locked(j, s) : TFHE_AMD_E_HIP;
    for (int k = 0; k < n_out && run == TFHE_AMD_OK && e == hipSuccess; ++k) {
        e = hipMemcpyAsync(out_a + (size_t)k * nb * kn, wa + (size_t)out_wires[k] * nb * kn, sizeof(int32_t) * nb * kn,
                           hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(out_b + (size_t)k * nb, wb + (size_t)out_wires[k] * nb, sizeof(int32_t) * nb,
                               hipMemcpyDeviceToHost, s);
    }
    const hipError_t sync = hipStreamSynchronize(s);   // before the buffers go, whatever happened
    (void)hipFree(wa);
    (void)hipFree(wb);
    if (run != TFHE_AMD_OK) return run;
    HIPCHK(e);
    HIPCHK(sync);
    return TFHE_AMD_OK;
}
