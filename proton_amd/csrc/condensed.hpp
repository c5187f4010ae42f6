// condensed.hpp -- tables and host entry points of the condensed (face-only) assembly, condensed.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_buf.hpp"
#include "face_system.hpp"
#include "structured_mesh.hpp"

namespace pa {

// what the condensed assembly kernels know of the mesh: the assembler's face tables (hho_assembly.hpp) plus the two
// cells of every local face (adj[2f], adj[2f+1]: lower cell id first; 0x7fffffff / -1 = none, equal = one cell)
struct CondMesh {
    const uint32_t *cell_faces;
    const int32_t *face_compress;
    const int32_t *adj;
    StructuredMesh sm;
    bool structured;
};

// face adjacency and the symbolic records of the owned faces, built on first use (cond_prepare)
struct CondTables {
    DeviceBuf<int32_t> adj;
    DeviceBuf<CondFace> cfaces;
    DeviceBuf<CondFaceLean> cfaces_lean;
    DeviceBuf<uint32_t> ncols, prefix;
    uint32_t nown = 0, owned_range = 0;
    int32_t p0 = 0;
    uint64_t total_cols = 0;                  // sum of the column-face counts of the owned faces
    bool ready() const { return prefix.get() != nullptr; }
};

// fills t's arrays (allocated by the caller: adj 2 nfaces_local, the others nown + 1); m.adj is taken from t
hipError_t cond_build_tables(hipStream_t stream, CondMesh m, uint32_t nfaces_local, uint32_t ncells, uint32_t owned_range,
                             int32_t p0, uint32_t nown, const CondTables &t);
// the owned rows of the face-only system from the view's condensed part (faces / lean, colprefix, nown)
hipError_t cond_pattern(hipStream_t stream, const FaceSystemView &v, int fbs, int64_t *rowptr, int32_t *colind);
hipError_t cond_fill(hipStream_t stream, const FaceSystemView &v, int fbs, const double *cond, const double *g, const double *halo,
                     double *values, double *rhs);
hipError_t cond_halo_pack(hipStream_t stream, const CondMesh &m, uint32_t first_cell, uint32_t ncells_row, int fbs, const double *cond,
                          const double *g, double *halo);
hipError_t cond_triplets(hipStream_t stream, const CondMesh &m, int num_cus, size_t first, size_t n, int fbs, const double *cond,
                         const double *g, int32_t *rows, int32_t *cols, double *vals, int32_t *rhs_rows, double *rhs_vals);
hipError_t cond_take_faces(hipStream_t stream, const CondMesh &m, size_t first, size_t n, int fbs, const double *solution,
                           const double *g, double *uF);
hipError_t cond_expand(hipStream_t stream, size_t ncells_local, size_t cell_base, size_t ncells_global, int cbs, size_t nface_dofs,
                       const double *uT, const double *xF, double *full);

}  // namespace pa
