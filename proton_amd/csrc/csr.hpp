// csr.hpp -- host entry point of csr.hip: COO triplet slots -> CSR with duplicates summed in push order.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace pa {

// slots with a negative row are skipped; *nnz_out (if given) = entries of the result, after the stream has drained
hipError_t csr_from_triplets(hipStream_t stream, size_t n, const int32_t *d_rows, const int32_t *d_cols, const double *d_vals,
                             size_t nrows, int64_t *d_rowptr, int32_t *d_colind, double *d_values, size_t *nnz_out);

}  // namespace pa
