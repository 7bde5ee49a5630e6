// keyring_internal.h — the key ring as keyring.cpp (gate and LUT batches) and
// keyring_circuit.cpp (circuits, §3.13) share it.  Internal, not part of the C ABI.
#pragma once
#include <mutex>
#include <vector>

#include "context.h"

struct TfheAmdKeyRing {
    std::vector<TfheAmdContext *> m;   // slot -> member (borrowed)
    int device = -1;
    void **d_fft = nullptr;            // [n_keys] the members' bk_fft (v6)
    void **d_v2 = nullptr;             // [n_keys] the members' bk_v2 (v4)
    std::mutex mu;                     // one call at a time: the tables below are the call's
    void *h_tab = nullptr, *d_tab = nullptr;   // the call's tables: pinned host copy, device copy
    size_t tab_bytes = 0;
    hipEvent_t up = nullptr;           // the last upload out of h_tab
    tfhe_amd::StreamFence fence;       // d_tab reuse across caller streams
    // the id under which circuits keep the device state of their runs on this ring (level tables, u
    // scratch): from the contexts' counter, so never a context's and never reused
    uint64_t uid = next_context_uid();
};

constexpr int kRingMaxKeys = 256;
