// l3d_model.h -- the sizes and the slicing that the stages on a flat model of 3D segments share (DESIGN §16-§19:
// project, associate, compare, merge; their host plumbing is l3d_model.hip, declared in l3d_ctx.h).  Plain C++17 without
// a HIP include (g++ compiles it for tests/test_model_slicing.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

namespace l3d {

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }   // device tables start at multiples of 256 bytes
// Offsets of tables packed one behind the other: take() hands out the next 256-aligned offset and moves behind the
// table, so that `at` is the size of everything taken so far.
struct Layout {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = up256(at); at = o + bytes; return o; }
};

constexpr uint32_t kSliceChunk = 256;    // references per chunk (= kCmpChunk of l3d_kernels.h)
// Slices of a walk of n_queries queries over n_refs references (both > 0), and the chunks per slice that go with them:
// a workgroup per (tile of queries, slice), bytes_per_cell bytes of partial results per (query, slice), which stay
// within budget -- fewer, longer slices where they would not.  The library's own choice (asked_chunks = 0) is ONE CHUNK
// PER SLICE: measured on C1 and C2 it is the fastest of the slicings tried or level with it, where a rule
// that aims at 1024 workgroups was 35 % slower at C2 (13 slices of 5 chunks on 65 tiles: 3.3 workgroups per compute
// unit, where seven fit).  No slice is empty and every chunk is covered, which the kernels rely on.
struct SlicePlan { uint32_t n_slices, slice_chunks; };
inline SlicePlan slice_plan(uint32_t n_queries, uint32_t n_refs, uint32_t asked_chunks, size_t bytes_per_cell, size_t budget) {
    const uint32_t n_chunks = (n_refs + kSliceChunk - 1) / kSliceChunk;
    const size_t cells = budget / (bytes_per_cell * (size_t)n_queries);
    const uint32_t cap = cells < 1 ? 1u : cells > n_chunks ? n_chunks : (uint32_t)cells;
    SlicePlan p;
    p.slice_chunks = asked_chunks ? (asked_chunks < n_chunks ? asked_chunks : n_chunks) : 1;
    p.n_slices = (n_chunks + p.slice_chunks - 1) / p.slice_chunks;
    if (p.n_slices <= cap) return p;
    p.slice_chunks = (n_chunks + cap - 1) / cap;
    p.n_slices = (n_chunks + p.slice_chunks - 1) / p.slice_chunks;
    return p;
}

// H x = rhs for a symmetric H of n <= kCholeskyMax rows, of which the upper triangle H[i * n + j], i <= j, is read, by a
// plain Cholesky factorisation H = L L^T, column by column, then the forward and the backward substitution: the loops
// DESIGN §23 writes out, which the alignment (n = 6 or 7) and the pose refinement of §27 (n = 6) share.  false: a pivot
// that is not finite and > 0, x untouched.
constexpr int kCholeskyMax = 7;
inline bool cholesky_solve(int n, const double* H, const double* rhs, double* x) {
    double L[kCholeskyMax][kCholeskyMax] = {}, y[kCholeskyMax], z[kCholeskyMax];
    for (int j = 0; j < n; ++j) {
        double p = H[j * n + j];
        for (int k = 0; k < j; ++k) p = p - L[j][k] * L[j][k];
        if (!(p > 0.0) || !std::isfinite(p)) return false;
        L[j][j] = std::sqrt(p);
        for (int i = j + 1; i < n; ++i) {
            double v = H[j * n + i];
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < n; ++i) {
        double v = rhs[i];
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < n; ++k) v = v - L[k][i] * z[k];
        z[i] = v / L[i][i];
    }
    for (int i = 0; i < n; ++i) x[i] = z[i];
    return true;
}

}  // namespace l3d
