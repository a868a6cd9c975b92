// sirconv_dropedge.hip — DropEdge (dgl.transforms.DropEdge, models/utils.py:96-102): the dropped graph's
// complete plan derived from the parent's, without a sort.
//
// A dropped graph's two row CSRs are order-preserving subsequences of the parent's, which are sorted
// already.  With keep(e) a bit per parent EDGE ID (a uint8 mask, or the counter hash of sirconv_dropout.h at
// element (e, 0)), three prefix sums decide everything:
//   id[e]  = kept ids below e              -> the survivor's new edge id (dgl.remove_edges: renumbered
//                                             0..E'-1 in ascending parent id)
//   d[i]   = kept dst-CSR positions below i -> its new dst-CSR position
//   s[i]   = kept src-CSR positions below i -> its new src-CSR position
// They are ONE scan of E + 1 {id, d, s} triples, in place (element E is the zero sentinel, so entry E
// holds the totals and entry i + 1 minus entry i is position i's flags).  Launches:
//   1. k_flags   : per position i: {keep(i), keep(eid_d[i]), keep(eid_s[i])}
//   2. scan      : hipcub::DeviceScan::ExclusiveScan, int adds
//   3. k_compact : per position i, for the kept ones: kept[id[i]] = i; col', eid' = id[eid[i]] of both
//                  CSRs; perm'[s[i]] = d[perm[i]] — the two lookups are the only gathers
//   4. k_child_deg: per row of either CSR: degree = scan[rowptr[r + 1]] - scan[rowptr[r]]
//   5. the builder's plan stage (run_plan_rows, sirconv_plan.hip) on each side: rowptr', items', splits',
//      counts.
// Integer only, deterministic; work is per edge position (a hub row is as parallel as any other); the one
// atomic is the plan stage's max-degree.  No allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "sirconv_internal.h"

namespace sir {
namespace {

struct Flag3 {
    int id, d, s;
};

struct Flag3Add {
    __host__ __device__ Flag3 operator()(const Flag3& a, const Flag3& b) const {
        return Flag3{a.id + b.id, a.d + b.d, a.s + b.s};
    }
};

// an id outside [0, E) (a malformed parent plan) reads slot 0 instead of memory it does not own
__device__ __forceinline__ int64_t in_range(int64_t e, int64_t E) { return (uint64_t)e < (uint64_t)E ? e : 0; }

template <bool HASH>
__device__ __forceinline__ int keep_bit(const uint8_t* __restrict__ keep, const Drop& d, int64_t e) {
    if constexpr (HASH) return !d.on() || drop_keep(d, drop_row_hash(d, e), 0);
    else return keep[e] != 0;
}

template <bool HASH>
__global__ void __launch_bounds__(256)
k_flags(const int64_t* __restrict__ eid_d, const int64_t* __restrict__ eid_s, const uint8_t* __restrict__ keep,
        Drop drop, int64_t E, Flag3* __restrict__ f) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > E) return;
    if (i == E) {
        f[i] = Flag3{0, 0, 0};
        return;
    }
    const Drop d = drop_resolve(drop);
    f[i] = Flag3{keep_bit<HASH>(keep, d, i), keep_bit<HASH>(keep, d, in_range(eid_d[i], E)),
                 keep_bit<HASH>(keep, d, in_range(eid_s[i], E))};
}

__global__ void __launch_bounds__(256)
k_compact(const Flag3* __restrict__ sc, int64_t E, const int* __restrict__ col_d, const int64_t* __restrict__ eid_d,
          const int* __restrict__ col_s, const int64_t* __restrict__ eid_s, const int* __restrict__ perm_s,
          int* __restrict__ col_d2, int64_t* __restrict__ eid_d2, int* __restrict__ col_s2,
          int64_t* __restrict__ eid_s2, int* __restrict__ perm_s2, int64_t* __restrict__ kept,
          int64_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    const Flag3 a = sc[i], b = sc[i + 1];
    if (b.id != a.id) kept[a.id] = i;
    if (b.d != a.d) {
        col_d2[a.d] = col_d[i];
        eid_d2[a.d] = sc[in_range(eid_d[i], E)].id;
    }
    if (b.s != a.s) {
        col_s2[a.s] = col_s[i];
        eid_s2[a.s] = sc[in_range(eid_s[i], E)].id;
        perm_s2[a.s] = sc[in_range(perm_s[i], E)].d;
    }
    if (i == E - 1) counts[8] = b.id;
}

// rows [0, n_d): the dst CSR; rows [n_d, n_d + n_s): the src CSR
__global__ void __launch_bounds__(256)
k_child_deg(const Flag3* __restrict__ sc, int64_t E, const int* __restrict__ rowptr_d, int64_t n_d,
            const int* __restrict__ rowptr_s, int64_t n_s, int* __restrict__ deg_d, int* __restrict__ deg_s) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_d + n_s) return;
    const bool dst = r < n_d;
    const int* rp = dst ? rowptr_d + r : rowptr_s + (r - n_d);
    const int64_t b = min(max((int64_t)rp[0], (int64_t)0), E);
    const int64_t e = min(max((int64_t)rp[1], b), E);
    if (dst) deg_d[r] = sc[e].d - sc[b].d;
    else deg_s[r - n_d] = sc[e].s - sc[b].s;
}

inline size_t up256(size_t x) { return (x + 255) & ~size_t(255); }
inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }

// workspace: scan triples | deg_d | deg_s | acc | off | cub temp
struct Layout {
    size_t sc, deg_d, deg_s, acc, off, temp, temp_bytes, total;
};

// Scan scratch, stated as a formula so that the workspace size needs no device: hipcub's look-back scan keeps
// a flag and two values (at most 16 B each here) per block of at least 64 items.  run_plan_drop compares it
// with what hipcub asks for before anything is launched.
inline size_t scan_temp_bound(int64_t n) { return up256((size_t)n) + 16384; }

void layout(int64_t n_d, int64_t n_s, int64_t E, Layout& L) {
    const int64_t n_max = n_d > n_s ? n_d : n_s;
    size_t o = 0;
    L.sc = o;    o += up256(sizeof(Flag3) * (size_t)(E + 1));
    L.deg_d = o; o += up256(sizeof(int) * (size_t)(n_d + 1));
    L.deg_s = o; o += up256(sizeof(int) * (size_t)(n_s + 1));
    L.acc = o;   o += plan_rows_acc_bytes(n_max);
    L.off = o;   o += plan_rows_acc_bytes(n_max);
    L.temp = o;
    L.temp_bytes = scan_temp_bound(E + 1 > n_max ? E + 1 : n_max);
    o += L.temp_bytes;
    L.total = o;
}

// what the three scans really need (a device query)
hipError_t scan_temp_needed(int64_t n_d, int64_t n_s, int64_t E, size_t* need) {
    size_t flag_bytes = 0, rows_d = 0, rows_s = 0;
    hipError_t err;
    if (E > 0) {
        err = hipcub::DeviceScan::ExclusiveScan(nullptr, flag_bytes, (const Flag3*)nullptr, (Flag3*)nullptr,
                                                Flag3Add(), Flag3{0, 0, 0}, (int)(E + 1));
        if (err != hipSuccess) return err;
    }
    if ((err = plan_rows_temp_bytes(n_d, &rows_d)) != hipSuccess) return err;
    if ((err = plan_rows_temp_bytes(n_s, &rows_s)) != hipSuccess) return err;
    *need = flag_bytes > rows_d ? flag_bytes : rows_d;
    if (rows_s > *need) *need = rows_s;
    return hipSuccess;
}

}  // namespace

int64_t plan_drop_workspace(int64_t n_dst_rows, int64_t n_src_rows, int64_t E) {
    Layout L;
    layout(n_dst_rows, n_src_rows, E, L);
    return (int64_t)L.total;
}

hipError_t run_plan_drop(const PlanDropArgs& a, void* ws, int64_t ws_bytes, hipStream_t st) {
    Layout L;
    layout(a.n_dst_rows, a.n_src_rows, a.E, L);
    size_t need = 0;
    hipError_t err = scan_temp_needed(a.n_dst_rows, a.n_src_rows, a.E, &need);
    if (err != hipSuccess) return err;
    if ((int64_t)L.total > ws_bytes || need > L.temp_bytes) return hipErrorInvalidValue;
    char* w = static_cast<char*>(ws);
    Flag3* sc = reinterpret_cast<Flag3*>(w + L.sc);
    int* deg_d = reinterpret_cast<int*>(w + L.deg_d);
    int* deg_s = reinterpret_cast<int*>(w + L.deg_s);
    void* temp = w + L.temp;
    const int64_t E = a.E, n_d = a.n_dst_rows, n_s = a.n_src_rows;
    // counts: {n_items, n_splits, n_slots, max_degree} of the dst CSR, of the src CSR, E'
    if ((err = hipMemsetAsync(a.counts, 0, 9 * sizeof(int64_t), st)) != hipSuccess) return err;
    if (E > 0) {
        if (a.keep != nullptr)
            hipLaunchKernelGGL(k_flags<false>, dim3(nblk(E + 1)), dim3(256), 0, st, a.eid_d, a.eid_s, a.keep, a.drop,
                               E, sc);
        else
            hipLaunchKernelGGL(k_flags<true>, dim3(nblk(E + 1)), dim3(256), 0, st, a.eid_d, a.eid_s, a.keep, a.drop,
                               E, sc);
        if ((err = hipGetLastError()) != hipSuccess) return err;
        size_t tb = L.temp_bytes;
        err = hipcub::DeviceScan::ExclusiveScan(temp, tb, sc, sc, Flag3Add(), Flag3{0, 0, 0}, (int)(E + 1), st);
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL(k_compact, dim3(nblk(E)), dim3(256), 0, st, sc, E, a.col_d, a.eid_d, a.col_s, a.eid_s,
                           a.perm_s, a.col_d2, a.eid_d2, a.col_s2, a.eid_s2, a.perm_s2, a.kept, a.counts);
        if ((err = hipGetLastError()) != hipSuccess) return err;
        if (n_d + n_s > 0) {
            hipLaunchKernelGGL(k_child_deg, dim3(nblk(n_d + n_s)), dim3(256), 0, st, sc, E, a.rowptr_d, n_d,
                               a.rowptr_s, n_s, deg_d, deg_s);
            if ((err = hipGetLastError()) != hipSuccess) return err;
        }
    } else {
        if ((err = hipMemsetAsync(deg_d, 0, sizeof(int) * (size_t)(n_d + 1), st)) != hipSuccess) return err;
        if ((err = hipMemsetAsync(deg_s, 0, sizeof(int) * (size_t)(n_s + 1), st)) != hipSuccess) return err;
    }
    if (n_d > 0)
        err = run_plan_rows(deg_d, n_d, a.chunk, w + L.acc, w + L.off, temp, L.temp_bytes, a.rowptr_d2, a.items_d2,
                            a.splits_d2, a.counts, st);
    else
        err = hipMemsetAsync(a.rowptr_d2, 0, sizeof(int), st);
    if (err != hipSuccess) return err;
    if (n_s > 0)
        return run_plan_rows(deg_s, n_s, a.chunk, w + L.acc, w + L.off, temp, L.temp_bytes, a.rowptr_s2, a.items_s2,
                             a.splits_s2, a.counts + 4, st);
    return hipMemsetAsync(a.rowptr_s2, 0, sizeof(int), st);
}

}  // namespace sir
