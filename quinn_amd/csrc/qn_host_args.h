// Host-side argument checks and workspace carving shared by the host code of every operator: the float64 extension operators
// (qn_curv.hip, qn_glm.hip, qn_kron.hip, qn_sobolev.hip) use both, the kernel families of the core operator (qn_mlp_sse_fwd /
// _fwdbwd: qn_fused.hip, qn_api.hip, qn_generic.hip, qn_rnet.hip, qn_fused_i8.hip, qn_wide_i8.hip) the carving.  Every check
// sets the error message and returns false; the caller picks the return code, so the order of an entry point's checks stays in
// its own body.  Not part of the C ABI.
#pragma once
#include "qn_common.h"

// NULL and residual-network descriptors; `family` names the refusing kernels ("the curvature kernels")
static inline bool qn_check_mlp_desc(const qn_desc* d, const char* who, const char* family) {
    if (!d) {
        qn_set_error("%s: NULL descriptor", who);
        return false;
    }
    if (d->kind != QN_KIND_MLP) {
        qn_set_error("%s: residual networks (RNet) are not supported by %s; an MLP descriptor is needed", who, family);
        return false;
    }
    return true;
}

// one member per blockIdx.y: the grid limit
static inline bool qn_check_members(int B, const char* who) {
    if (B <= 0 || B > 65535) {
        qn_set_error("%s: need 1 <= B <= 65535 members (B=%d)", who, B);
        return false;
    }
    return true;
}

static inline bool qn_check_row_idx(const int32_t* row_idx, int N, int Nb, const char* who) {
    if (!row_idx && Nb != N) {
        qn_set_error("%s: without row_idx Nb (%d) must equal N (%d)", who, Nb, N);
        return false;
    }
    return true;
}

static inline bool qn_check_workspace(const void* workspace, size_t workspace_bytes, size_t need, const char* who) {
    if (!workspace || workspace_bytes < need) {
        qn_set_error("%s: workspace of %zu bytes, need %zu", who, workspace_bytes, need);
        return false;
    }
    return true;
}

// Carves a workspace into qn_align'ed blocks: take() returns the block's byte offset, `total` is the size so far.  A kernel
// family fills a struct of such offsets in ONE layout function; its size query returns that struct's `total` and its run
// function takes every pointer from the same struct (qn_ws_at), so the two cannot disagree.
struct qn_ws_carver {
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t off = total;
        total += qn_align(bytes);
        return off;
    }
    template <class T> size_t take(size_t n) { return take(n * sizeof(T)); }
    size_t take_doubles(size_t n) { return take<double>(n); }
};

// offset of a block that a layout does not hold (a forward-only workspace has no gradient slabs): qn_ws_at gives NULL for it
constexpr size_t QN_WS_NONE = ~size_t(0);

template <class T = double>
static inline T* qn_ws_at(void* workspace, size_t off) {
    return off == QN_WS_NONE ? nullptr : reinterpret_cast<T*>(static_cast<char*>(workspace) + off);
}
