// Internal declarations of the SIREConv edge kernels (sirconv_eedge.hip), shared with the C-ABI TU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sir {

// fp32 rows only; every feature pointer 16-B aligned with leading dimensions that are multiples of 4
struct EEdgeArgs {
    const int* rowptr;
    const int* col;
    const int32_t* items;
    int64_t n_items;
    const int32_t* splits;
    int64_t n_splits;
    int H;
    const float* Q;  int64_t ldq;      // forward: destination rows
    const float* K;  int64_t ldk;      // forward: gathered source rows
    const float* Eh; int64_t lde;      // forward: gathered edge rows, n_erows of them
    int64_t n_erows;
    const int* eidx;                   // dst-CSR position -> edge row (NULL: the position itself)
    const float* norm_row;
    const float* norm_col;
    float slope;
    float* S;  int64_t lds;            // forward output
    uint64_t* mask_out;                // forward: sign mask of z (sir_mask_words layout) or NULL
    float* partial;                    // forward: split rows' partial sums
    const uint64_t* mask_in;           // edge-term backward
    const float* G;  int64_t ldg;      // edge-term backward: gradient rows of the destinations
    float* dE; int64_t ldde;           // edge-term backward output, n_erows rows
};

// agg: AGG_SUM / AGG_MEAN / AGG_SYM (backward: SUM / SYM), act: ACT_RELU / ACT_LEAKY.
// hipErrorInvalidValue with *why set: a shape / layout the kernels do not take.
hipError_t run_eedge_fwd(const EEdgeArgs& a, int agg, int act, hipStream_t st, const char** why);
hipError_t run_eedge_bwd_e(const EEdgeArgs& a, int agg, int act, hipStream_t st, const char** why);

}  // namespace sir
