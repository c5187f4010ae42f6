// fictdom_condensed.hpp -- host entry points of fictdom_condensed.hip: the cut cells of the fictitious-domain system condensed
// to their face unknowns, and their cell unknowns recovered, in double-double.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pa {

// the records [upper triangle of S | g] of the cut cells, written over rows cut_cells[cc] of the cell-major record array `cond`
// (pa_condensed_ops_batch's layout); info_cut[cc] = 200 + j + 1 for a failed pivot j, 0 otherwise (may be null)
hipError_t fdcond_cut_records(hipStream_t stream, int face_deg, int max_blocks, uint32_t ncut, const uint32_t *cut_cells, const double *cut_lc,
                              const double *cut_rhs, double *cond, int32_t *info_cut);
// u_T of the cut cells into uT (cell-major, ncells x cbs) from uF (ncells x 4 fbs: the face values of every cell, Dirichlet faces
// carrying the boundary data)
hipError_t fdcond_cut_recover(hipStream_t stream, int face_deg, int max_blocks, uint32_t ncut, const uint32_t *cut_cells, const double *cut_lc,
                              const double *cut_rhs, const double *uF, double *uT);
// rhs of the uncut cells outside `where` zeroed in the copy dst (n = ncells x cbs entries); src null: zeros
hipError_t fdcond_masked_rhs(hipStream_t stream, size_t ncells, int cbs, const int8_t *cell_loc, int where, const double *src, double *dst);
hipError_t fdcond_copy(hipStream_t stream, size_t n, const double *src, double *dst);

}  // namespace pa
