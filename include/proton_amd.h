/*
 * proton_amd.h -- C ABI of the MI355X-native HHO local-operator assembly path.
 *
 * The reference (OmarDuran/ProtoN) is a header-only C++ template library with no
 * FFI; its interface for this path is a set of per-cell function templates.  This
 * ABI is the batched, device-side equivalent that a binding of those templates
 * calls.  Each entry point cites the reference interface it replaces
 * (paths relative to the reference root).  Plain pointers and sizes only; no
 * C++/torch types; no exceptions cross this boundary (int status codes).
 *
 * Pointers named d_* are DEVICE pointers (hipMalloc'd or e.g. torch tensors'
 * data_ptr()); everything else is host memory.  All matrices are column-major
 * (Eigen's default, which the reference returns), batched cell-major:
 * entry (row i, col j) of cell c lives at  base[c * rows*cols + j*rows + i].
 *
 * Threading: one context per device/stream; calls on a context are ordered by
 * its HIP stream and are asynchronous with respect to the host unless stated.
 */
#ifndef PROTON_AMD_H
#define PROTON_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_ABI_VERSION 5

/* status codes (reference: C++ exceptions / silent NaNs) */
enum {
    PA_OK = 0,
    PA_ERR_INVALID_ARG = 1,
    PA_ERR_INVALID_DEGREE = 2,     /* hho_degree_info pair not instantiated                       */
    PA_ERR_QUADRATURE = 3,         /* "Quadrature order too high" quadratures.hpp:245-246, incl. the
                                      rules[8] hole of the fan quadrature (quadratures_dunavant.hpp:129) */
    PA_ERR_HIP = 4,                /* a HIP runtime call failed; see pa_last_error()               */
    PA_ERR_NO_MESH = 5,
    PA_ERR_NOT_SPD = 6,            /* some cell had a non-positive Cholesky pivot (Eigen LLT: silent) */
    PA_ERR_COMM = 7                /* RCCL missing or an RCCL call failed; see pa_comm_last_error()  */
};

/* integrate() overloads: quadratures.hpp:311-375 (quad_mesh, tensor Gauss) and
 * quadratures.hpp:377-402 (poly_mesh, 4-triangle fan + Dunavant). */
enum { PA_QUAD_TENSOR = 0, PA_QUAD_FAN = 1 };
/* stabilization choice: none / make_hho_naive_stabilization hho.hpp:99-148 /
 * make_hho_fancy_stabilization hho.hpp:155-237 */
enum { PA_STAB_NONE = 0, PA_STAB_NAIVE = 1, PA_STAB_FANCY = 2 };
/* built-in source terms evaluated on the device (the reference passes a C++ lambda) */
enum {
    PA_FN_SAMPLED = 0,             /* values supplied per quadrature point by the caller            */
    PA_FN_SIN_SIN_RHS = 1,         /* 2 pi^2 sin(pi x) sin(pi y)   convergence_test.cpp:100-102,
                                      cuthho_square.cpp:846-848                                     */
    PA_FN_SIN_SIN_SOL = 2,         /* sin(pi x) sin(pi y)          convergence_test.cpp:104-106     */
    PA_FN_OBSTACLE_RHS = 3,        /* obstacle.cpp:67-74  (r0 = 0.7)                                */
    PA_FN_OBSTACLE_SOL = 4,        /* obstacle.cpp:76-81                                            */
    PA_FN_ONE = 5
};

typedef struct pa_context pa_context;

/* hho_degree_info (utils.hpp:62-111) as plain ints */
typedef struct { int32_t cell_deg, face_deg, rec_deg; } pa_degree_info;
/* hho_degree_info(size_t) utils.hpp:71-73 */
pa_degree_info pa_degree_info_equal(int degree);
/* hho_degree_info(size_t cd, size_t fd) utils.hpp:75-95; *fell_back (may be NULL) is set
 * when the pair is invalid and the reference "reverts to equal-order" */
pa_degree_info pa_degree_info_make(int cd, int fd, int *fell_back);

/* sizes: cell_basis::size bases.hpp:191-194, face_basis::size bases.hpp:287-290 */
typedef struct {
    int32_t rbs, cbs, fbs, msize;      /* msize = cbs + 4 fbs                                   */
    int32_t oper_rows;                 /* rbs - 1 (hho.hpp:52-53)                               */
    int32_t cell_qps, face_qps;        /* points of integrate(cell, 2 recdeg) / (face, 2 facdeg) */
} pa_sizes;
int pa_sizes_for(pa_degree_info di, int quad_kind, pa_sizes *out);

/* ---- context ------------------------------------------------------------------------ */
/* `stream` is the hipStream_t every call of the context is enqueued on; NULL is HIP's default
 * (null) stream -- which is what torch.cuda.current_stream().cuda_stream reports for torch's
 * default stream.  With own_stream != 0 `stream` is ignored and the context creates (and later
 * destroys) a non-blocking stream of its own. */
int pa_context_create(int device, void *stream, int own_stream, pa_context **out);
int pa_context_destroy(pa_context *ctx);
int pa_context_synchronize(pa_context *ctx);
/* on != 0: pa_cut_local_ops_batch / pa_cut_rhs_sampled_batch run on a side stream of the context, next to whatever
 * is enqueued on its main stream AFTER them -- call them before pa_local_ops_batch so that the few cut cells
 * (one wavefront each, a long serial chain) overlap the uncut cells' kernels (cuthho_square.cpp:883-900 handles
 * both kinds in one loop).  Their outputs are ordered only before pa_cut_merge and pa_context_synchronize.
 * Off by default: everything on the one stream, in call order.  (Pays only when the main stream's kernels leave
 * room: next to the persistent local-operator grid of a 512^2 mesh it measured 8 % slower than the plain sequence.) */
int pa_context_set_cut_overlap(pa_context *ctx, int on);
const char *pa_last_error(pa_context *ctx);      /* text of the last HIP failure, "" if none  */
/* The record buffer of the local-operator calls (see pa_local_ops_batch) grows on demand up to a cap -- 4 GiB, or what
 * pa_context_set_record_cap says (>= 1 MiB; larger ranges of cells run in equal pieces); calls that write local matrices
 * run in pieces of at most 192 Ki cells anyway (135 MB of records at k = 2: a piece's records stay in the Infinity Cache
 * between its two kernels) -- and stays with the
 * context for reuse.  pa_context_trim waits for the context's stream and gives it back to the device. */
int pa_context_set_record_cap(pa_context *ctx, size_t bytes);
/* The columns up to which the whole-mesh table builders pa_condensed_coarse[_query] and pa_interface_condensed_coarse[_query]
 * serve a table (the coarse spaces of solver_cg.hpp:63-144's preconditioner, cuthho_square.cpp:915-919): PA_COARSE_MAX_NODES by
 * default -- what the exactly solved level of pa_coarse_precond_* takes --, up to PA_SMOOTHED_MAX_NODES for the tables of smoothed
 * levels (pa_smoothed_level_*); 0 restores the default, a larger value is PA_ERR_INVALID_ARG.  The builders of a slab's rows
 * (pa_condensed_rows_coarse, pa_interface_rows_coarse) and pa_coarse_precond_* keep PA_COARSE_MAX_NODES. */
int pa_context_set_coarse_table_cap(pa_context *ctx, size_t max_columns);
int pa_context_trim(pa_context *ctx);
int pa_abi_version(void);

/* device-memory helpers so a non-torch host (the C++ header, a cgo/JNI caller) needs no HIP */
int pa_malloc(pa_context *ctx, size_t bytes, void **d_out);
int pa_free(pa_context *ctx, void *d_ptr);
int pa_memcpy_h2d(pa_context *ctx, void *d_dst, const void *src, size_t bytes);   /* synchronous */
int pa_memcpy_d2h(pa_context *ctx, void *dst, const void *d_src, size_t bytes);   /* synchronous */
int pa_memset(pa_context *ctx, void *d_dst, int value, size_t bytes);

/* ---- mesh ----------------------------------------------------------------------------
 * Replaces the mesh<T,4,...> storage the kernels consume: msh.points (basic_mesh.hpp:222)
 * and cell.ptids (basic_mesh.hpp:51).  points: np x 2 doubles (x,y), cell_ptids: nc x 4
 * uint32 in the reference's CCW order.  The arrays are copied to the device. */
int pa_mesh_upload(pa_context *ctx, const double *points, size_t npoints,
                   const uint32_t *cell_ptids, size_t ncells);
/* Same, but the arrays already live on the device and are borrowed (not copied, not freed). */
int pa_mesh_attach_device(pa_context *ctx, const double *d_points, size_t npoints,
                          const uint32_t *d_cell_ptids, size_t ncells);
/* Structured generator mesh_impl<T,4>(mesh_init_params) basic_mesh.hpp:230-298, built on
 * the device: points (min + i*h), cells {p, p+1, p+Nx+2, p+Nx+1}, cell id = j*Nx + i.
 * row_begin/row_end select the block of cell rows [row_begin,row_end) this context owns
 * (multi-GPU partition); cell index 0 of the context is global cell row_begin*Nx. */
int pa_mesh_generate(pa_context *ctx, size_t Nx, size_t Ny,
                     double min_x, double max_x, double min_y, double max_y,
                     size_t row_begin, size_t row_end);
int pa_mesh_counts(pa_context *ctx, size_t *npoints, size_t *ncells);
/* Replaces the coordinates of a mesh the context owns (pa_mesh_upload / pa_mesh_generate) and keeps its connectivity and
 * numbering: msh.points edited in place (the commented-out node perturbation of convergence_test.cpp:176-187; a general
 * quadrilateral mesh with the generator's closed-form face numbering, whole or as a slab of cell rows -- d_points then holds
 * the slab's node rows row_begin .. row_end).  d_points: npoints x 2 doubles on the device, copied on the context's stream. */
int pa_mesh_set_points(pa_context *ctx, const double *d_points, size_t npoints);

/* ---- the hot path --------------------------------------------------------------------
 * For cells [first, first+n) of the uploaded mesh computes, per cell,
 *   (oper, data) = make_hho_laplacian(msh, cl, di)                 hho.hpp:32-96
 *   stab         = make_hho_{naive,fancy}_stabilization(...)       hho.hpp:99-148 / 155-237
 *   lc           = data + stab                                     convergence_test.cpp:212
 * Any of the d_* outputs may be NULL (not written).  Shapes per cell:
 *   d_oper (rbs-1) x msize, d_data/d_stab/d_lc msize x msize, d_info one int32
 *   (0, or 1+index of the first non-positive Cholesky pivot: 100+ for the cell-mass
 *   factorization of the fancy stabilization).
 * Asynchronous on the context's stream.  Two kernels per call: a one-thread-per-cell pre-pass and the
 * cooperative kernel, which meet in a record buffer the CONTEXT owns (grown on demand, at most 4 GiB --
 * pa_context_set_record_cap -- larger ranges run in equal pieces; released by pa_context_trim / pa_context_destroy).  Calls on one
 * context are serialized by its stream, so the buffer needs no locking; use one context per stream. */
int pa_local_ops_batch(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind,
                       size_t first, size_t n,
                       double *d_oper, double *d_data, double *d_stab, double *d_lc,
                       int32_t *d_info);

/* make_rhs(msh, cl, degree, f, di) utils.hpp:153-174 for every cell in [first, first+n):
 * d_rhs[c][cbs(degree)].  fn = PA_FN_*; with PA_FN_SAMPLED d_fvals holds f at the
 * quadrature points of integrate(cell, 2*(degree+dinc)), n x nqp doubles in the
 * reference's point order (pa_cell_quadrature_points returns the points). */
int pa_cell_rhs_batch(pa_context *ctx, int degree, int dinc, int quad_kind, int fn,
                      const double *d_fvals, size_t first, size_t n, double *d_rhs);
/* integrate(msh, cl, degree) quadratures.hpp:311-402: d_xyw[c][nqp][3] = (x, y, weight) */
int pa_cell_quadrature_points(pa_context *ctx, int degree, int quad_kind,
                              size_t first, size_t n, double *d_xyw, int32_t *nqp_out);

/* Static condensation of the cell unknowns (the reference has none):
 *   S = A_FF - A_FT A_TT^-1 A_TF,  g = -A_FT A_TT^-1 f_T,
 *   rec = [ A_TT^-1 f_T | -A_TT^-1 A_TF ]   (cbs x (1 + 4 fbs)),  u_T = rec[:,0] + rec[:,1:] u_F.
 * d_lc: n x msize^2, d_rhs: n x cbs (may be NULL = 0).  Outputs may be NULL. */
int pa_static_condensation_batch(pa_context *ctx, pa_degree_info di, size_t n,
                                 const double *d_lc, const double *d_rhs,
                                 double *d_S, double *d_g, double *d_rec, int32_t *d_info);
/* Same, with the symmetric Schur complement stored as its upper triangle, column-packed:
 * d_Sp[c][j*(j+1)/2 + i] = S(i,j), i <= j, nf*(nf+1)/2 values per cell (the multi-GPU exchange
 * format: values only, indices closed-form). */
int pa_static_condensation_packed_batch(pa_context *ctx, pa_degree_info di, size_t n,
                                        const double *d_lc, const double *d_rhs,
                                        double *d_Sp, double *d_g, int32_t *d_info);

/* ---- condensed mode: static condensation fused into the local-operator pass ---------------------
 * The north star's hot path ends in the static condensation of the cell unknowns (SURVEY section 8 row
 * A15; the reference has none: its assemblers keep cell AND face unknowns, hho.hpp:331).  In this mode
 * lc = data + stab never reaches HBM: the kernel eliminates the cbs cell unknowns of every cell on chip
 * and writes, per cell, one packed record of  nf (nf + 1) / 2 + nf  doubles (nf = 4 fbs):
 *   the upper triangle of  S = A_FF - A_FT A_TT^-1 A_TF,  column-packed (S(i,j), i <= j, at j(j+1)/2 + i),
 *   then  g = -A_FT A_TT^-1 f_T.
 * d_rhs: f_T = make_rhs (utils.hpp:153-174), n x cbs, or NULL (= 0).  d_cond: n x (nf(nf+1)/2 + nf).
 * d_info as pa_local_ops_batch; 200 + j flags pivot j of A_TT.  stab_kind must not be PA_STAB_NONE
 * (A_TT = data_TT is singular on the constants, hho.hpp:93). */
int pa_condensed_ops_batch(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind,
                           size_t first, size_t n, const double *d_rhs, double *d_cond, int32_t *d_info);
/* The same pass run for the recovery of the eliminated unknowns once the face unknowns are known:
 *   u_T = A_TT^-1 (f_T - A_TF u_F)      d_uF: n x nf (pa_condensed_take_faces), d_uT: n x cbs. */
int pa_condensed_recover_batch(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind,
                               size_t first, size_t n, const double *d_rhs, const double *d_uF,
                               double *d_uT, int32_t *d_info);

/* The face-only global system the condensed records assemble into: the reference's numbering
 * (hho.hpp:305-331, 362-379) without its cbs * ncells block of cell unknowns -- unknown k of
 * non-Dirichlet face F sits at compress_table[F] * fbs + k. */
typedef struct {
    uint64_t system_size;        /* fbs * num_other_faces                                            */
    uint64_t num_other_faces;
    int32_t nf, cond_doubles;    /* 4 fbs; nf (nf + 1) / 2 + nf                                     */
    /* row partition: the context OWNS the rows of the faces of its cell rows' blocks (for every cell
     * row its bottom and vertical faces; the horizontals closing the slab on top belong to the slab
     * above): the contiguous row range [row_begin, row_end) of the global system */
    uint64_t row_begin, row_end;
    uint64_t nnz_owned;          /* stored entries of the owned rows                                 */
    uint64_t halo_cells;         /* cells whose top face belongs to the slab above (Nx, or 0 for the
                                    topmost slab): pa_condensed_halo_pack writes that many rows      */
    int32_t halo_doubles;        /* doubles per halo row: fbs * (nf + 1)                             */
    int32_t has_below;           /* != 0: the slab's bottom faces also receive the contribution of the
                                    slab below: pa_condensed_csr_fill expects d_halo_below            */
} pa_condensed_info;
int pa_condensed_query(pa_context *ctx, pa_degree_info di, pa_condensed_info *out);
/* The row partition alone, in closed form, for the slab [row_begin, row_end) of the Nx x Ny generator mesh: what
 * pa_condensed_query reports for such a context, without a context or a device (nnz_owned is left 0).  Lets a driver
 * size its buffers and its exchange before any rank has touched its GPU. */
int pa_condensed_partition_info(size_t Nx, size_t Ny, size_t row_begin, size_t row_end, pa_degree_info di,
                                pa_condensed_info *out);

/* assembler::assemble (hho.hpp:344-406) on the condensed blocks, cells [first, first+n): per cell nf^2
 * triplet slots in the reference's push order restricted to the face unknowns (slot i*nf + j for face
 * rows i, j of the local matrix), row = col = -1 where either face is Dirichlet; d_rhs_rows / d_rhs_vals
 * n x nf: g_i minus the Dirichlet columns times the boundary data (hho.hpp:401).  d_g from
 * pa_dirichlet_data_batch or NULL. */
int pa_condensed_triplets_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n,
                                const double *d_cond, const double *d_g,
                                int32_t *d_rows, int32_t *d_cols, double *d_vals,
                                int32_t *d_rhs_rows, double *d_rhs_vals);
/* The same system built directly in CSR from the mesh's face adjacency -- no triplets, no sort.
 * Symbolic phase, once per mesh and degree: d_rowptr (row_end - row_begin + 1 entries, int64, starting
 * at 0) and d_colind (nnz_owned global column ids, ascending within a row). */
int pa_condensed_csr_pattern(pa_context *ctx, pa_degree_info di, int64_t *d_rowptr, int32_t *d_colind);
/* Numeric phase, once per assembly: d_values (nnz_owned) and d_rhs (row_end - row_begin) from the
 * records of ALL the context's cells (d_cond: ncells x cond_doubles).  Contributions of the two cells of
 * a face are added lower cell id first, the order setFromTriplets sums the triplets above in: values are
 * bit-identical to pa_csr_from_triplets of pa_condensed_triplets_batch.  d_halo_below: the rows packed by
 * the slab below (has_below), else NULL. */
int pa_condensed_csr_fill(pa_context *ctx, pa_degree_info di, const double *d_cond, const double *d_g,
                          const double *d_halo_below, double *d_values, double *d_rhs);
/* What the slab above needs of this slab: for every cell of the top cell row the fbs rows of its top
 * face -- fbs x nf values S(2 fbs + k, :) with Dirichlet columns already moved to the right-hand side,
 * then the fbs right-hand-side contributions; halo_cells x halo_doubles doubles.  These rows are the
 * whole multi-GPU exchange of an assembly step (pa_comm_* below). */
int pa_condensed_halo_pack(pa_context *ctx, pa_degree_info di, const double *d_cond, const double *d_g, double *d_halo);
/* take_local_data (hho.hpp:408-449) restricted to the faces: d_uF n x nf from the face-only solution
 * (system_size values), Dirichlet faces from d_g. */
int pa_condensed_take_faces(pa_context *ctx, pa_degree_info di, size_t first, size_t n,
                            const double *d_solution, const double *d_g, double *d_uF);
/* The reference's full solution vector (cells first, then compressed faces; hho.hpp:331) from the
 * recovered cell unknowns (ncells x cbs, the context's cells) and the face-only solution: what
 * assembler::take_local_data and the postprocessing expect.  d_full: cbs * ncells_global + system_size;
 * a slab writes its own cells and (d_xF != NULL) the face part. */
int pa_condensed_expand_solution(pa_context *ctx, pa_degree_info di, const double *d_uT, const double *d_xF,
                                 double *d_full);

/* ---- assembler<Mesh> (hho.hpp:252-463) ---------------------------------------------------
 * Face connectivity.  pa_mesh_generate builds it in closed form; for an uploaded mesh supply
 * msh.faces as the reference holds them (basic_mesh.hpp:114-137, sorted by (lo,hi) point ids):
 * cell_faces[c][4] = offset(msh, fc) of faces(msh, cl) (basic_geom.hpp:183-212, order bottom,
 * right, top, left), face_pts[f][2] = fc.ptids (lo, hi), face_is_dirichlet[f] =
 * fc.is_boundary && fc.bndtype == DIRICHLET.  Host arrays; copied. */
int pa_mesh_set_faces(pa_context *ctx, const uint32_t *cell_faces, const uint32_t *face_pts,
                      const uint8_t *face_is_dirichlet, size_t nfaces);

typedef struct {
    uint64_t system_size;        /* cbs * ncells + fbs * num_other_faces        hho.hpp:331      */
    uint64_t ncells_global;      /* cells of the whole mesh                                       */
    uint64_t cell_base;          /* global id of the context's cell 0 (row partition)             */
    uint64_t nfaces_local;       /* rows of the context's face tables (d_g has nfaces_local x fbs) */
    uint64_t face_base;          /* global id of local face 0                                      */
    uint64_t num_other_faces;    /* non-Dirichlet faces of the whole mesh       hho.hpp:305-307   */
} pa_assembler_info;
int pa_assembler_query(pa_context *ctx, pa_degree_info di, pa_assembler_info *out);

/* Dirichlet data of every boundary face, mass.llt().solve(rhs) of the boundary function
 * (hho.hpp:381-386): d_g[f][fbs], zeros for non-Dirichlet faces.  fn = PA_FN_*; with
 * PA_FN_SAMPLED d_fvals holds the function at the face quadrature points (nfaces_local x
 * (face_deg+1), the points come from pa_face_quadrature_points). */
int pa_dirichlet_data_batch(pa_context *ctx, int face_deg, int fn, const double *d_fvals, double *d_g);
/* integrate(msh, fc, 2*face_deg) quadratures.hpp:404-432: d_xyw[f][face_deg+1][3]; face_deg <= 7: closed-form rules to
 * five nodes, golub_welsch's (quadratures.hpp:32-75, ascending nodes) to eight
 * (pass face_deg + di for the points of a degree-increased rule, utils.hpp:185) */
int pa_face_quadrature_points(pa_context *ctx, int face_deg, double *d_xyw);

/* assembler::assemble (hho.hpp:344-406) for cells [first, first+n): per cell msize^2 triplet
 * slots in the reference's push order (slot i*msize + j for local row i, column j); a slot whose
 * row or column belongs to a Dirichlet face holds row = col = -1.  Row/column indices are the
 * reference's int triplet indices (Eigen::Triplet<T>).  The right-hand-side updates of
 * hho.hpp:401,405 are returned per local row: d_rhs_rows[c][msize] (global row or -1) and
 * d_rhs_vals[c][msize]; RHS = scatter-add of those.  d_lc: n x msize^2, d_rhs: n x cbs or NULL,
 * d_g from pa_dirichlet_data_batch or NULL (homogeneous). */
int pa_triplets_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n,
                      const double *d_lc, const double *d_rhs, const double *d_g,
                      int32_t *d_rows, int32_t *d_cols, double *d_vals,
                      int32_t *d_rhs_rows, double *d_rhs_vals);

/* The same system -- assembler<Mesh>'s own numbering, cell AND face unknowns (system_size = cbs * ncells + fbs *
 * num_other_faces, hho.hpp:331), i.e. what assemble (hho.hpp:344-406) + finalize = setFromTriplets (hho.hpp:451-455)
 * leave in `LHS` / `RHS` -- built DIRECTLY in CSR from the mesh's face adjacency: no triplets, no sort.  The span the
 * reference's drivers print as "Matrix assembly" (apps/cuthho/cuthho_square.cpp:881-905,
 * apps/convergence_test/convergence_test.cpp:201-217) is pa_local_ops_batch + pa_cell_rhs_batch + pa_assembler_csr_fill.
 * Whole-mesh contexts only (a slab of a partitioned mesh assembles the face-only system: pa_condensed_*).
 * Symbolic phase, once per mesh and degree: nrows = system_size, nnz; d_rowptr nrows + 1 (int64), d_colind nnz (int32,
 * ascending within a row; may be NULL).  Numeric phase, once per assembly: d_values nnz, d_RHS nrows (may be NULL) from
 * d_lc (ncells x msize^2), d_rhs (ncells x cbs or NULL), d_g (pa_dirichlet_data_batch or NULL).  Structure and values
 * bit-identical to pa_csr_from_triplets of pa_triplets_batch, d_RHS to the scatter-add of its d_rhs_vals in cell order. */
typedef struct { uint64_t nrows, nnz; } pa_assembler_csr_info;
int pa_assembler_csr_query(pa_context *ctx, pa_degree_info di, pa_assembler_csr_info *out);
int pa_assembler_csr_pattern(pa_context *ctx, pa_degree_info di, int64_t *d_rowptr, int32_t *d_colind);
int pa_assembler_csr_fill(pa_context *ctx, pa_degree_info di, const double *d_lc, const double *d_rhs, const double *d_g,
                          double *d_values, double *d_RHS);

/* make_hho_laplacian + stabilization + assembler::assemble + finalize in one pass per cell (hho.hpp:32-237, :344-406,
 * :451-455): the reference turns a cell's local matrix into global entries in the loop iteration that formed it, and so does
 * this entry -- the local-operator kernel writes d_values / d_RHS of the pattern pa_assembler_csr_query / _pattern describe
 * straight from its on-chip image of lc; no ncells x msize^2 buffer exists unless d_lc asks for one (the layout of
 * pa_local_ops_batch; callers need it again for the energy error, convergence_test.cpp:283-300).  All cells of the context
 * (whole-mesh contexts only, refused as pa_assembler_csr_fill refuses a slab); the (degree pair, quadrature, stabilization)
 * combinations and error codes of pa_condensed_ops_batch; in pieces under pa_context_set_record_cap as pa_local_ops_batch.
 * d_rhs (ncells x cbs or NULL), d_g (pa_dirichlet_data_batch or NULL), d_RHS nrows (may be NULL), d_info ncells (may be NULL).
 * Contract: d_values and d_RHS are BIT-IDENTICAL to pa_assembler_csr_fill fed with the d_lc this call returns and the same
 * d_rhs / d_g, with or without d_lc and from call to call.  A face's own diagonal block and right-hand side take one addend
 * per adjacent cell; they are added onto entries the call zeroes first, a two-term sum that does not depend on arrival order.
 * Every other entry is written exactly once and nothing else of d_values is touched. */
int pa_assembler_csr_assemble(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind,
                              const double *d_rhs, const double *d_g,
                              double *d_values, double *d_RHS,
                              double *d_lc /* may be NULL */, int32_t *d_info /* may be NULL */);

/* assembler::take_local_data (hho.hpp:408-449) for cells [first, first+n): d_out n x msize =
 * the cell's dofs of `d_solution` (system_size values), Dirichlet faces filled from d_g
 * (pa_dirichlet_data_batch; NULL = homogeneous). */
int pa_take_local_data_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n,
                             const double *d_solution, const double *d_g, double *d_out);

/* project_function(msh, cl, hdi, f, di) (utils.hpp:199-227) for cells [first, first+n):
 * d_out n x msize = L2 projection of f on the cell basis (mass and rhs at degree
 * 2*(cell_deg + dinc)) followed by the projections on the four faces (degree
 * 2*(face_deg + dinc)).  fn = PA_FN_*; with PA_FN_SAMPLED d_cell_fvals holds f at the points of
 * pa_cell_quadrature_points(2*(cell_deg+dinc)) for those cells and d_face_fvals at the points
 * of pa_face_quadrature_points(face_deg + dinc) for every face of the context. d_info (n, may be
 * NULL): first non-positive pivot of the cell mass matrix (+1), 0 if SPD. */
int pa_project_function_batch(pa_context *ctx, pa_degree_info di, int quad_kind, int dinc, int fn,
                              const double *d_cell_fvals, const double *d_face_fvals,
                              size_t first, size_t n, double *d_out, int32_t *d_info);
/* d_out[c] = (u_c - v_c)^T lc_c (u_c - v_c) for n cells (the energy-error summand of
 * convergence_test.cpp:283-300 / obstacle.cpp:202-213); d_v may be NULL (v = 0). */
int pa_energy_form_batch(pa_context *ctx, pa_degree_info di, size_t n, const double *d_lc, const double *d_u,
                         const double *d_v, double *d_out);

/* ---- obstacle_assembler<Mesh> (hho.hpp:471-751) ---------------------------------------------
 * These entry points need the whole mesh on the context (no row slab).
 * Constructor tables (hho.hpp:538-578): d_in_A ncells flags (is_in_set_A), d_A_ct / d_B_ct
 * ncells int32: position among the cells outside / inside the active set, -1 otherwise.
 * *num_I / *num_A (host) receive the two counts. */
int pa_obstacle_tables(pa_context *ctx, const uint8_t *d_in_A, int32_t *d_A_ct, int32_t *d_B_ct,
                       size_t *num_I, size_t *num_A);
/* obstacle_assembler::assemble (hho.hpp:609-695) for cells [first, first+n).  Slot layout:
 * msize^2 + 1 slots per cell, slot i*msize + j = lhs(i,j) in the reference's push order, the last
 * slot the multiplier coupling (row cell*cbs, column num_I*cbs + num_other*fbs + B_ct[cell], 1.0)
 * of active cells (hho.hpp:688-693); rows/cols = -1 for slots the reference does not push.
 * Rows are not compressed (cell rows at cell + i, hho.hpp:631: exact for cbs = 1, the only case
 * obstacle.cpp:51 uses), columns are (hho.hpp:625,645).  d_gamma: one value per cell
 * (hho.hpp:677).  d_rhs_rows / d_rhs_vals: n x msize as in pa_triplets_batch. */
int pa_obstacle_triplets_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n,
                               const double *d_lc, const double *d_rhs, const double *d_g, const double *d_gamma,
                               const uint8_t *d_in_A, const int32_t *d_A_ct, const int32_t *d_B_ct, size_t num_I,
                               int32_t *d_rows, int32_t *d_cols, double *d_vals,
                               int32_t *d_rhs_rows, double *d_rhs_vals);
/* obstacle_assembler::expand_solution (hho.hpp:698-744): d_alpha ncells*cbs + nfaces*fbs (cells,
 * then ALL faces, Dirichlet ones from d_g), d_beta ncells*cbs multipliers. */
int pa_obstacle_expand_solution(pa_context *ctx, pa_degree_info di, const double *d_solution, const double *d_g,
                                const double *d_gamma, const uint8_t *d_in_A, const int32_t *d_A_ct,
                                const int32_t *d_B_ct, size_t num_I, double *d_alpha, double *d_beta);
/* free take_local_data(msh, cl, di, expanded_solution) (hho.hpp:753-782): d_out n x msize */
int pa_obstacle_take_local_data_batch(pa_context *ctx, pa_degree_info di, size_t first, size_t n,
                                      const double *d_expanded, double *d_out);

/* obstacle_assembler::assemble + finalize (hho.hpp:609-695, :746-750) for ALL cells of a whole-mesh context -- the cell loop
 * of the active-set iteration, obstacle.cpp:147-158 -- built DIRECTLY in CSR: no triplets, no sort, no host scatter.  Cell
 * degree 0 only (cbs = 1, what obstacle.cpp:51 uses): there the system is the plain assembler's system of the pair (0, face_deg)
 * with its columns renumbered by the active set, an order-preserving compaction of the pattern of pa_assembler_csr_pattern.
 * Inputs as pa_obstacle_triplets_batch with first = 0, n = ncells (d_rhs ncells or NULL, d_g pa_dirichlet_data_batch or NULL;
 * d_in_A / d_A_ct / d_B_ct / num_I of pa_obstacle_tables).  Outputs sized by pa_assembler_csr_query(ctx, di): d_rowptr
 * nrows + 1 (int64), d_colind / d_values with room for its nnz (the count reached when the active set is empty), d_RHS nrows
 * (may be NULL); *nnz (host) receives the stored count = that nnz - fbs * #{(non-Dirichlet face, active adjacent cell)} after a
 * stream synchronise, as in pa_csr_from_triplets.  Nothing at or beyond *nnz is written.
 * Contract: d_rowptr, d_colind[:*nnz], d_values[:*nnz] and *nnz are BIT-IDENTICAL to pa_csr_from_triplets of
 * pa_obstacle_triplets_batch with the same arguments; d_RHS equals the scatter-add of that call's d_rhs_vals in cell order onto
 * zeros.  Refusals, before any output buffer is touched: a NULL pointer other than d_rhs / d_g / d_RHS, num_I > ncells, 2^31
 * rows and more, a row slab ("whole mesh" in pa_last_error): PA_ERR_INVALID_ARG; a degree outside the tables or
 * cell_deg != 0 (the overlapping cell rows of hho.hpp:631 for cbs > 1 stay with the triplet route): PA_ERR_INVALID_DEGREE. */
int pa_obstacle_csr_assemble(pa_context *ctx, pa_degree_info di,
                             const double *d_lc, const double *d_rhs /* or NULL */, const double *d_g /* or NULL */,
                             const double *d_gamma, const uint8_t *d_in_A, const int32_t *d_A_ct, const int32_t *d_B_ct, size_t num_I,
                             int64_t *d_rowptr, int32_t *d_colind, double *d_values, double *d_RHS /* or NULL */, size_t *nnz);

/* The solve of that system -- obstacle.cpp:170-175, Eigen::SparseLU in the reference -- on the device, in place on the arrays
 * pa_obstacle_csr_assemble wrote.  The system of obstacle_assembler::assemble (hho.hpp:609-695) keeps its rows where the plain
 * assembler has them (cell rows at the cell index, face rows behind them) and compacts its columns: inactive cells at [0, num_I),
 * face unknowns up to nk = nrows - num_A, multipliers at [nk, nrows).  An active cell's row holds its multiplier with
 * coefficient 1 and no other row holds one (hho.hpp:688-693).  Hence the kept rows (inactive cells in d_A_ct order, then all face
 * rows) against the columns below nk are a symmetric positive definite block K, and each remaining row defines one multiplier.
 * K goes to the reference's conjugate gradient (pa_conjugated_gradient, which stands in for the SparseLU) through a row map --
 * no copy of d_colind / d_values is made --, then x[column of the multiplier] = b_i - sum_j A_ij x_j for every active row i.
 * Inputs: the arrays and d_RHS of pa_obstacle_csr_assemble for (ctx, di), the tables and num_I of pa_obstacle_tables, the solver
 * parameters of pa_conjugated_gradient.  Output: d_x, nrows values in the reference's solution layout, what
 * pa_obstacle_expand_solution reads; the three results of pa_conjugated_gradient (host, each may be NULL).
 * Contract: d_x[:nk], *exit_reason, *iterations and *relative_residual are BIT-IDENTICAL to pa_conjugated_gradient on K
 * extracted into arrays of its own; a multiplier differs from its evaluation in another order by rounding only.  nk = 0 (every
 * cell active, every face Dirichlet) returns converged after 0 iterations.  A solve that does not converge is not an error: the
 * status is PA_OK, *exit_reason says why, d_x holds the last iterate and its multipliers.
 * Refusals, before anything is written: a NULL pointer other than the three results, num_I > ncells, a row slab ("whole mesh" in
 * pa_last_error): PA_ERR_INVALID_ARG; a degree outside the tables or cell_deg != 0: PA_ERR_INVALID_DEGREE.
 * Returns after the stream has drained. */
int pa_obstacle_block_solve(pa_context *ctx, pa_degree_info di,
                            const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values, const double *d_RHS,
                            const uint8_t *d_in_A, const int32_t *d_A_ct, const int32_t *d_B_ct, size_t num_I,
                            double convergence_threshold, double divergence_threshold, size_t max_iter, int apply_preconditioner,
                            double *d_x, int32_t *exit_reason, size_t *iterations, double *relative_residual);

/* The active set of the next iteration and the stopping norm of this one (obstacle.cpp:133-142 and :193) in one pass:
 *   d_in_A[i] = (d_beta[i] + c * (d_alpha[i] - d_gamma[i])) < 0    for the ncells cells (cell degree 0: one value per cell),
 * the difference, the product and the sum each rounded on its own as the reference's expression is (no fused multiply-add: it
 * can flip the flag of a cell whose exact value is a rounding error away from zero; a value of exactly zero is inactive);
 * *num_A = active cells; *changed = cells whose flag differs from d_in_A_prev (NULL: from the empty set; may be d_in_A itself);
 * *step_norm = || d_alpha_prev - d_alpha ||_2 over all ncells + fbs * nfaces values (d_alpha_prev NULL: zeros), summed by a
 * block-tree reduction in a fixed order: the same bits from run to run.  The three results are host pointers, each may be NULL.
 * Whole-mesh contexts, cell degree 0, as pa_obstacle_csr_assemble.  Returns after the stream has drained. */
int pa_obstacle_active_set_update(pa_context *ctx, pa_degree_info di, double c,
                                  const double *d_alpha, const double *d_beta, const double *d_gamma,
                                  const double *d_alpha_prev /* or NULL */, const uint8_t *d_in_A_prev /* or NULL */,
                                  uint8_t *d_in_A, size_t *num_A, size_t *changed, double *step_norm);

/* The primal-dual active set loop of run_hho_obstacle (obstacle.cpp:117-197) in one call, on the reference's own system (not a
 * condensed one), every array on the device; the host reads a few scalars per outer iteration.  From alpha = 0, beta = 1
 * (obstacle.cpp:98-99), until max_outer systems have been solved: pa_obstacle_active_set_update, pa_obstacle_tables,
 * pa_obstacle_csr_assemble, pa_obstacle_block_solve, pa_obstacle_expand_solution, and the step norm of :193 (formed by the
 * update that also yields the next active set); the loop ends converged when that norm is below outer_tol.
 * The CSR arrays (pa_assembler_csr_query's sizes), the solver's vectors, the row map and the solution buffers are allocated
 * once per call and freed on every path out.
 * Inputs: d_lc (pa_local_ops_batch for the pair (0, face_deg)), d_rhs (ncells or NULL), d_g (pa_dirichlet_data_batch or NULL),
 * d_gamma (ncells: the obstacle at the barycentres).  Outputs: d_alpha (ncells + fbs * nfaces), d_beta (ncells), d_in_A (ncells:
 * the active set of the last system solved), *info, and two optional host arrays of max_outer entries, filled up to
 * info->outer_iterations: the number of active cells and the conjugate gradient's iterations of every system.
 * A conjugate gradient that does not converge ends the loop: the status is PA_OK, info->converged = 0, info->cg_exit_reason
 * holds pa_conjugated_gradient's code (1 diverged, 2 max_iter), d_alpha / d_beta are those of the last completed iteration
 * (alpha = 0, beta = 1 if the first solve failed) and d_in_A is the active set they give, the one whose system was not solved.
 * Refusals, before anything is written: NULL d_lc / d_gamma / params / d_alpha / d_beta / d_in_A / info, max_outer = 0, a row
 * slab: PA_ERR_INVALID_ARG; a degree outside the tables or cell_deg != 0: PA_ERR_INVALID_DEGREE. */
typedef struct {
    double c;                          /* obstacle.cpp:101: 1.0 */
    size_t max_outer;                  /* systems solved at most; the reference's loop: 50 (obstacle.cpp:119) */
    double outer_tol;                  /* the reference's 1e-7 (obstacle.cpp:193) */
    double cg_convergence_threshold, cg_divergence_threshold;
    size_t cg_max_iter;                /* 0 = 20 * nk of the system at hand */
    int32_t apply_preconditioner;      /* Jacobi */
} pa_obstacle_solve_params;
typedef struct {
    uint64_t outer_iterations;         /* systems solved */
    uint64_t cg_iterations;            /* over all of them */
    double last_step_norm;             /* || alpha_prev - alpha ||_2 of the last completed iteration */
    int32_t converged;                 /* last_step_norm < outer_tol */
    int32_t cg_exit_reason;            /* of the last solve */
} pa_obstacle_solve_info;
int pa_obstacle_solve(pa_context *ctx, pa_degree_info di,
                      const double *d_lc, const double *d_rhs /* or NULL */, const double *d_g /* or NULL */, const double *d_gamma,
                      const pa_obstacle_solve_params *params,
                      double *d_alpha, double *d_beta, uint8_t *d_in_A, pa_obstacle_solve_info *info,
                      size_t *num_A_history /* or NULL */, size_t *cg_iterations_history /* or NULL */);

/* SparseMatrix::setFromTriplets (hho.hpp:451-455, :746-750; cuthho_square.cpp:1437-1441) on the
 * device: nslots triplet slots (a negative row or column = a slot the assembler did not push) ->
 * CSR with duplicates summed in push order.  d_rowptr nrows+1 (int64), d_colind / d_values with room
 * for nslots entries (the worst case); *nnz (host) receives the number of stored entries.
 * Column indices are ascending within a row.  nslots < 2^31. */
int pa_csr_from_triplets(pa_context *ctx, size_t nslots, const int32_t *d_rows, const int32_t *d_cols, const double *d_vals,
                         size_t nrows, int64_t *d_rowptr, int32_t *d_colind, double *d_values, size_t *nnz);

/* conjugated_gradient(A, b, x, cg_params) (src/core/core_bits/solver_cg.hpp:45-144; the solver of
 * run_cuthho_interface, cuthho_square.cpp:1737-1743) on the CSR matrix of pa_csr_from_triplets.  Same
 * recurrences and exit tests, in the reference's order: *exit_reason = 0 converged (relative residual
 * below convergence_threshold), 2 max_iter reached (iter > max_iter), 1 diverged (relative residual above
 * divergence_threshold).  apply_preconditioner: Jacobi.  x starts from zero (solver_cg.hpp:73).  The dot
 * products are tree reductions, not Eigen's sequential sums: iterates agree to rounding, not bitwise. */
int pa_conjugated_gradient(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind,
                           const double *d_values, const double *d_b, double *d_x,
                           double convergence_threshold, double divergence_threshold, size_t max_iter,
                           int apply_preconditioner, int32_t *exit_reason, size_t *iterations, double *relative_residual);

/* ---- a patch preconditioner for that conjugate gradient --------------------------------------------------
 * Where solver_cg.hpp:77-80 keeps 1 / diag(A) and solver_cg.hpp:63-144 multiplies the residual by it, these keep the inverse
 * of the dense diagonal block of every PATCH of rows and apply the additive Schwarz sum
 *     z = sum_p R_p^T (R_p A R_p^T)^-1 R_p r
 * (the solve they serve: cuthho_square.cpp:915-919 on the face-only system).  The patch table is a CSR-like pair:
 * d_patch_ptr (npatches + 1, int64, starting at 0) and d_patch_rows (d_patch_ptr[npatches] global row indices, int32).
 * A patch holds 1 to PA_PATCH_MAX_ROWS rows, none twice; a row may lie in several patches and every row lies in at least
 * one.  A table that breaks one of these -- an index out of range, a repeated row, a patch size outside 1..16, an uncovered
 * row -- is refused with PA_ERR_INVALID_ARG and text in pa_last_error(), checked on the device before anything is indexed
 * with it, and no output buffer is touched (d_scratch is no output).  Callers own the device memory. */
#define PA_PATCH_MAX_ROWS 16
typedef struct {
    uint64_t entries;            /* d_patch_ptr[npatches]                                                        */
    int32_t max_patch_rows;      /* the largest patch; every factor takes max_patch_rows (max_patch_rows + 1) / 2 */
    int32_t lanes_per_patch;     /* 4, 8 or 16: the lanes that share a patch in the factor and apply kernels      */
    uint64_t factor_doubles;     /* doubles of d_factors                                                          */
    uint64_t slot_ints;          /* int32 of d_slots: nrows + 1 + entries                                         */
    uint64_t scratch_bytes;      /* bytes of d_scratch (the patch-major results of an apply, the build's counters) */
} pa_patch_precond_info;
/* solver_cg.hpp:63-144, cuthho_square.cpp:915-919: what a table needs; reads d_patch_ptr only (sizes within 1..16, else
 * PA_ERR_INVALID_ARG).  Waits for the stream. */
int pa_patch_precond_query(pa_context *ctx, size_t nrows, size_t npatches, const int64_t *d_patch_ptr, pa_patch_precond_info *out);
/* The set-up of solver_cg.hpp:63-144 (its lines 77-80) for patches (cuthho_square.cpp:915-919): validates the table, builds d_slots (per row the places of
 * its contributions in the patch-major buffer, ascending = in patch order) and factors every patch: A_p gathered from the
 * CSR arrays (columns ascending within a row; an absent entry is zero), Cholesky in plain double, the packed lower triangle
 * of L^-1 into d_factors.  d_info (npatches): 0, or j + 1 for the first non-positive pivot j of the patch; *failed_patches
 * (host, may be NULL) counts them, and any makes the call return PA_ERR_NOT_SPD.  Waits for the stream. */
int pa_patch_precond_factor(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                            size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows, double *d_factors,
                            int32_t *d_slots, void *d_scratch, int32_t *d_info, size_t *failed_patches);
/* The preconditioner's product of solver_cg.hpp:63-144 (its lines 84 and 126) for patches (cuthho_square.cpp:915-919): d_z = sum_p R_p^T A_p^-1 R_p d_r with
 * the table, d_factors, d_slots and d_scratch of a pa_patch_precond_factor that returned PA_OK.  Every patch writes its
 * results to a patch-major buffer and every row sums its contributions in ascending patch order: no floating-point atomics,
 * the same bits from call to call. */
int pa_patch_precond_apply(pa_context *ctx, size_t nrows, size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows,
                           const double *d_factors, const int32_t *d_slots, void *d_scratch, const double *d_r, double *d_z);
/* conjugated_gradient (solver_cg.hpp:63-144; the solve of cuthho_square.cpp:915-919) with the patch preconditioner: the
 * arguments and the three results of pa_conjugated_gradient with the patch table in place of apply_preconditioner; the same
 * recurrences, exit tests and exit order, z an explicit vector.  The factors live for the call.  A refused table:
 * PA_ERR_INVALID_ARG; a patch with a failed pivot: PA_ERR_NOT_SPD before the first iteration; d_x is untouched by both. */
int pa_conjugated_gradient_patch(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind,
                                 const double *d_values, const double *d_b, double *d_x,
                                 size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows,
                                 double convergence_threshold, double divergence_threshold, size_t max_iter,
                                 int32_t *exit_reason, size_t *iterations, double *relative_residual);
/* The patch tables of the face-only system of pa_condensed_csr_pattern (the Poisson and the fictitious-domain systems;
 * assembler::assemble hho.hpp:344-406 numbers its faces, the solve is cuthho_square.cpp:915-919 / solver_cg.hpp:63-144).
 * PA_PATCH_FACE: one patch per non-Dirichlet face, its fbs rows.  PA_PATCH_CELL: one patch per cell with at least one
 * non-Dirichlet face, in cell order, the rows of its non-Dirichlet faces in the cell's face order bottom, right, top, left
 * (up to 4 fbs, overlapping).  Whole-mesh contexts; a slab is refused with PA_ERR_INVALID_ARG as pa_assembler_csr_fill
 * refuses one.  The query gives the sizes of d_patch_ptr (*npatches + 1) and d_patch_rows (*entries). */
enum { PA_PATCH_FACE = 0, PA_PATCH_CELL = 1 };
int pa_condensed_patches_query(pa_context *ctx, pa_degree_info di, int kind, size_t *npatches, size_t *entries);
int pa_condensed_patches(pa_context *ctx, pa_degree_info di, int kind, int64_t *d_patch_ptr, int32_t *d_patch_rows);

/* ---- a Galerkin coarse level next to the patches --------------------------------------------------------
 * The patch sum has no global information: its iteration count grows with 1 / h.  These add one coarse level, solved exactly:
 *     z = (accumulate ? z : 0) + P (P^T A P)^-1 P^T r
 * The coarse space is a caller-owned table P (nrows x ncoarse) in CSR: d_p_ptr (nrows + 1, int64, starting at 0), d_p_cols
 * (int32) and d_p_vals (double).  A row holds 0 to PA_COARSE_MAX_ROW_ENTRIES entries, its columns ascend without repeats and lie
 * within [0, ncoarse), its values are finite; ncoarse runs from 1 to PA_COARSE_MAX_NODES.  A table that breaks one of these is
 * refused with PA_ERR_INVALID_ARG and text in pa_last_error(), checked on the device before anything is indexed with it, and no
 * output buffer is touched (d_scratch is no output).  Callers own the device memory. */
#define PA_COARSE_MAX_ROW_ENTRIES 4
#define PA_COARSE_MAX_NODES 4096
typedef struct {
    uint64_t entries;            /* d_p_ptr[nrows]                                                                     */
    uint64_t pt_bytes;           /* bytes of d_pt: P^T in CSR (row pointer, fine rows ascending within a row, values)   */
    uint64_t factor_doubles;     /* doubles of d_factor: ncoarse (ncoarse + 1) / 2, the packed lower triangle of L^-1    */
    uint64_t scratch_bytes;      /* bytes of d_scratch (the coarse vectors of an apply, the work space of the factor)    */
} pa_coarse_precond_info;
/* solver_cg.hpp:63-144, cuthho_square.cpp:915-919: what a table needs; reads d_p_ptr only (ncoarse within 1..4096 and rows of
 * 0..4 entries, else PA_ERR_INVALID_ARG).  Waits for the stream. */
int pa_coarse_precond_query(pa_context *ctx, size_t nrows, size_t ncoarse, const int64_t *d_p_ptr, pa_coarse_precond_info *out);
/* The set-up of solver_cg.hpp:63-144 (its lines 77-80) for the coarse level (cuthho_square.cpp:915-919): validates the table,
 * builds P^T into d_pt, forms A_c = P^T A P -- W = A P with at most 16 columns per row (more: PA_ERR_INVALID_ARG), then every
 * coarse row's lower triangle summed in a fixed order by the lane that owns the column, and mirrored: d_coarse_matrix (ncoarse^2,
 * may be NULL) is exactly symmetric --, takes its Cholesky factor in plain double and stores the packed lower triangle of L^-1
 * into d_factor.  The first non-positive pivot j gives *pivot = j + 1 (host, may be NULL; 0 otherwise) and PA_ERR_NOT_SPD.
 * Waits for the stream. */
int pa_coarse_precond_factor(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                             size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols, const double *d_p_vals, void *d_pt,
                             double *d_factor, void *d_scratch, double *d_coarse_matrix, int32_t *pivot);
/* The preconditioner's product of solver_cg.hpp:63-144 (its lines 84 and 126) for the coarse level (cuthho_square.cpp:915-919):
 * d_z = (accumulate ? d_z : 0) + P L^-T L^-1 P^T d_r with the table, d_pt, d_factor and d_scratch of a pa_coarse_precond_factor
 * that returned PA_OK.  Restriction: a fixed lane-strided order per coarse row, then a fixed reduction tree; two packed
 * triangular products; a gather of at most 4 terms per row.  No floating-point atomics, the same bits from call to call. */
int pa_coarse_precond_apply(pa_context *ctx, size_t nrows, size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols,
                            const double *d_p_vals, const void *d_pt, const double *d_factor, void *d_scratch, int accumulate,
                            const double *d_r, double *d_z);
/* conjugated_gradient (solver_cg.hpp:63-144; the solve of cuthho_square.cpp:915-919) with z = (patch sum) + (coarse term): the
 * arguments and the three results of pa_conjugated_gradient_patch plus the coarse table; the same recurrences, exit tests and
 * exit order.  The factors live for the call.  Refusals leave d_x untouched: of the patch table first, then of the coarse table
 * (PA_ERR_INVALID_ARG), then PA_ERR_NOT_SPD of either level before the first iteration. */
int pa_conjugated_gradient_patch_coarse(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind,
                                        const double *d_values, const double *d_b, double *d_x,
                                        size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows,
                                        size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols, const double *d_p_vals,
                                        double convergence_threshold, double divergence_threshold, size_t max_iter,
                                        int32_t *exit_reason, size_t *iterations, double *relative_residual);
/* The coarse table of the face-only system of pa_condensed_csr_pattern (the Poisson and the fictitious-domain systems; the
 * solve is cuthho_square.cpp:915-919 / solver_cg.hpp:63-144), built on the device: bilinear hats on every H-th mesh line.
 *   Coarse lines, per direction with N cells: the vertex indices 0, H, 2 H, .. below N, and N (H >= 1; the last interval is
 *   shorter if H does not divide N).  The 1-D hat of line l_j at vertex index i: 1 at l_j, (double)(i - l_(j-1)) / (double)(l_j -
 *   l_(j-1)) on the left interval, (double)(l_(j+1) - i) / (double)(l_(j+1) - l_j) on the right one, 0 elsewhere; the 2-D hat is
 *   phi = wx * wy, one rounding.  Hats live in index space: the table does not change with pa_mesh_set_points.
 *   Coarse nodes: the crossings of interior lines (the boundary is Dirichlet), row-major, jy outer, jx inner.
 *   Entries (face basis bases.hpp:253-279: monomials in ep, -1 at the face's first point a, +1 at its second point b): for
 *   compressed face q and every node with phi(a) != 0 or phi(b) != 0, row q fbs gets 0.5 * (phi(a) + phi(b)), row q fbs + 1
 *   (fbs >= 2) gets 0.5 * (phi(b) - phi(a)) when that is not zero; the rows of higher modes are empty.
 *   PA_COARSE_ONE: as above.  PA_COARSE_BY_SIDE (needs pa_cut_preprocess, else PA_ERR_NO_MESH): a face wholly on the side
 *   opposite to `where` is in part 1, every other face in part 0; a node's hat becomes up to two columns, each restricted to one
 *   part's faces; all part-0 columns come first, then the part-1 columns, each in node order; empty columns are dropped.
 * Whole-mesh structured contexts; a slab is refused as pa_condensed_patches refuses one.  No interior node, or more than
 * PA_COARSE_MAX_NODES columns: PA_ERR_INVALID_ARG with H and the count in pa_last_error().  The query gives ncoarse and the
 * size of d_p_cols / d_p_vals (*entries); d_p_ptr takes system rows + 1. */
enum { PA_COARSE_ONE = 0, PA_COARSE_BY_SIDE = 1 };
int pa_condensed_coarse_query(pa_context *ctx, pa_degree_info di, int H, int parts, int where, size_t *ncoarse, size_t *entries);
int pa_condensed_coarse(pa_context *ctx, pa_degree_info di, int H, int parts, int where, int64_t *d_p_ptr, int32_t *d_p_cols,
                        double *d_p_vals);

/* ---- smoothed hat levels next to the patches and the exact level: the additive multilevel form ------------
 * One exactly solved level is bound to PA_COARSE_MAX_NODES columns by its dense factor, so its H grows with the mesh and the
 * iteration count with H / h.  A SMOOTHED level is a coarse table whose Galerkin matrix is replaced by its diagonal:
 *     z = (accumulate ? z : 0) + P D^-1 P^T r,   D = diag(P^T A P),   d_j = sum_i P_ij (sum_k A_ik P_kj)
 * With smoothed levels on nested hat spaces (H = 2, 4, 8, ..) below one small exact level,
 *     z = sum_p R_p^T A_p^-1 R_p r + sum_l P_l D_l^-1 P_l^T r + P_c (P_c^T A P_c)^-1 P_c^T r,
 * the count stops growing with 1 / h.  The table format and row rules are those of pa_coarse_precond_* (rows of 0 to
 * PA_COARSE_MAX_ROW_ENTRIES entries, columns ascending within [0, ncoarse), finite values), with ncoarse from 1 to
 * PA_SMOOTHED_MAX_NODES: there is no dense matrix.  A table that breaks a rule is refused with PA_ERR_INVALID_ARG and text in
 * pa_last_error(), checked on the device before anything is indexed with it, and no output buffer is touched (d_scratch is no
 * output).  Every level prolongs straight to the fine rows: there is no table between levels.
 * Sums: entry e of a column (by fine row ascending) goes to slot e mod 64; a slot adds its entries in ascending order with fused
 * multiply-adds; the 64 slots are added by the xor tree 32, 16, 8, 4, 2, 1.  A column is owned by a wavefront or by a quarter of
 * one (lanes_per_column, chosen from the mean column length: 16 up to 32 entries, else 64); the bits do not depend on the choice.
 * No floating-point atomics: the same bits from call to call. */
#define PA_SMOOTHED_MAX_NODES (1u << 24)
#define PA_MULTILEVEL_MAX_LEVELS 8
typedef struct {
    uint64_t entries;            /* d_p_ptr[nrows]                                                                     */
    uint64_t pt_bytes;           /* bytes of d_pt: P^T in CSR (row pointer, fine rows ascending within a row, values)   */
    uint64_t dinv_doubles;       /* doubles of d_dinv: ncoarse                                                          */
    uint64_t scratch_bytes;      /* bytes of d_scratch (the coarse vector of an apply, the work space of the set-up)    */
    int32_t lanes_per_column;    /* 16 or 64                                                                            */
} pa_smoothed_level_info;
/* solver_cg.hpp:63-144, cuthho_square.cpp:915-919: what a smoothed level needs; reads d_p_ptr only (ncoarse within
 * 1..PA_SMOOTHED_MAX_NODES and rows of 0..4 entries, else PA_ERR_INVALID_ARG).  Waits for the stream. */
int pa_smoothed_level_query(pa_context *ctx, size_t nrows, size_t ncoarse, const int64_t *d_p_ptr, pa_smoothed_level_info *out);
/* The set-up of solver_cg.hpp:63-144 (its lines 77-80: the inverse diagonal, here of P^T A P) for a smoothed level: validates the
 * table, builds P^T into d_pt -- the entries keyed by (column, entry index) and radix-sorted, linear in the entries whatever the
 * columns' lengths --, forms d_j in the order stated above (row i of A walked in its entry order, column j looked up in row k of
 * P) and stores 1 / d_j into d_dinv.  A column whose d_j is not a positive finite number, an empty column included: *column =
 * j + 1 for the first such j (host, may be NULL; 0 otherwise) and PA_ERR_NOT_SPD; d_dinv is then not written (d_pt is work space,
 * not a result).  Waits for the stream. */
int pa_smoothed_level_setup(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values,
                            size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols, const double *d_p_vals, void *d_pt,
                            double *d_dinv, void *d_scratch, int32_t *column);
/* The preconditioner's product of solver_cg.hpp:63-144 (its lines 84 and 126) for a smoothed level: d_z = (accumulate ? d_z : 0)
 * + P D^-1 P^T d_r with the table, d_pt, d_dinv and d_scratch of a pa_smoothed_level_setup that returned PA_OK: one restriction
 * scaled by d_dinv, one gather of at most 4 terms per row added in entry order. */
int pa_smoothed_level_apply(pa_context *ctx, size_t nrows, size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols,
                            const double *d_p_vals, const void *d_pt, const double *d_dinv, void *d_scratch, int accumulate,
                            const double *d_r, double *d_z);
typedef struct {
    size_t ncoarse;
    const int64_t *d_p_ptr;
    const int32_t *d_p_cols;
    const double *d_p_vals;
} pa_coarse_table;
/* conjugated_gradient (solver_cg.hpp:63-144; the solve of cuthho_square.cpp:915-919) with the multilevel z above: the arguments
 * and the three results of pa_conjugated_gradient_patch, `levels` (a HOST array of nlevels smoothed tables, 0 to
 * PA_MULTILEVEL_MAX_LEVELS; NULL only with nlevels = 0) and `exact` (the table of the exactly solved level as
 * pa_conjugated_gradient_patch_coarse takes it; NULL: none).  The same recurrences, exit tests and exit order.  The terms of z are
 * added in the order patches, levels 0, 1, .., exact level; the gathers of all levels share one pass over z, which also forms the
 * partial sums of r . z.  The factors and the D^-1 vectors live for the call.  Refusals leave d_x untouched, in this order: the
 * patch table, each level's table in the caller's order (its index in pa_last_error()), the exact table (PA_ERR_INVALID_ARG);
 * then, before the first iteration, PA_ERR_NOT_SPD of the patches, of a level (its index and the column in pa_last_error()) or of
 * the exact level (whose product A P is judged with its factor).  nlevels = 0: d_x and the three results are
 * pa_conjugated_gradient_patch_coarse's bit for bit, and pa_conjugated_gradient_patch's with exact = NULL as well.  One rank: the
 * row-partitioned solver (pa_conjugated_gradient_rows_patch_coarse) takes no smoothed levels. */
int pa_conjugated_gradient_multilevel(pa_context *ctx, size_t nrows, const int64_t *d_rowptr, const int32_t *d_colind,
                                      const double *d_values, const double *d_b, double *d_x,
                                      size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows,
                                      size_t nlevels, const pa_coarse_table *levels, const pa_coarse_table *exact,
                                      double convergence_threshold, double divergence_threshold, size_t max_iter,
                                      int32_t *exit_reason, size_t *iterations, double *relative_residual);

/* ---- cutHHO (fictitious domain, `cuthho_square -f`) -----------------------------------------
 * circle_level_set / line_level_set, apps/cuthho/cuthho_square.cpp:56-124 */
typedef struct { int32_t kind; double radius, alpha, beta, cut_y; } pa_level_set;   /* kind 0 circle, 1 line */
enum { PA_LOC_NEGATIVE = 0, PA_LOC_POSITIVE = 1, PA_LOC_ON_INTERFACE = 2 };          /* element_location */

/* Builds the generator mesh (cuthho_poly_mesh, basic_mesh.hpp:321-403) and runs the host
 * preprocessing of cuthho_square.cpp:2036-2052 with node displacement (-D, the default):
 * detect_node_position, detect_cut_faces, move_nodes, detect_cut_faces, detect_cut_cells,
 * refine_interface(refsteps).  The displaced points become the context's mesh.  Errors the
 * reference throws ("invalid number of cuts in cell", "concave poly", "interface not found in
 * search range") are returned as PA_ERR_INVALID_ARG with the text in pa_last_error(). */
int pa_cut_preprocess(pa_context *ctx, size_t Nx, size_t Ny, double min_x, double max_x, double min_y, double max_y,
                      const pa_level_set *ls, int refsteps);
/* The same for the slab of cell rows [row_begin, row_end) of a row partition ("cut cells are distributed
 * by the same row rule"): the host preprocessing runs over the WHOLE mesh on every rank (deterministic: every rank tags and
 * displaces the same nodes), the context keeps the slab -- its displaced node rows, the tags of its cells and its own cut
 * cells, in ascending cell order.  Cell index 0 of the context is global cell row_begin * Nx (as pa_mesh_generate);
 * pa_cut_query reports the slab's cells; pa_cut_query_tags still reports the whole mesh.  Everything per cell works on a
 * slab (pa_cut_local_ops_batch, pa_cut_uncut_rhs_batch, pa_cut_merge, pa_cut_merge_condensed, pa_cut_interface_ops_batch,
 * pa_cut_interface_uncut_batch); the interface_assembler's numbering (pa_interface_*) and pa_cut_agglo_query need a
 * whole-mesh context and return PA_ERR_INVALID_ARG on a slab. */
int pa_cut_preprocess_rows(pa_context *ctx, size_t Nx, size_t Ny, double min_x, double max_x, double min_y, double max_y,
                           const pa_level_set *ls, int refsteps, size_t row_begin, size_t row_end);
/* The agglomeration branch of the same preprocessing (`-A`, cuthho_square.cpp:2039-2044): no node
 * displacement.  The reference then only CLASSIFIES the cut cells (detect_cell_agglo_set); its
 * agglomerate_cells is dead code (cuthho_square.cpp:1525-1621).  All operators of this library
 * work on the resulting mesh as on the displaced one. */
int pa_cut_preprocess_agglomeration(pa_context *ctx, size_t Nx, size_t Ny, double min_x, double max_x, double min_y,
                                    double max_y, const pa_level_set *ls, int refsteps);
/* detect_cell_agglo_set (cuthho_geom.hpp:163-273, threshold 0.3): agglo_set ncells (host),
 * 0 UNDEF, 1 T_OK, 2 T_KO_NEG, 3 T_KO_POS (cuthho_mesh.hpp's cell_agglo_set order), and
 * make_neighbors_info (cuthho_geom.hpp:343-370; O(cells^2) there, closed form here): neighbors
 * ncells x 8 cell ids sharing a point, ascending, -1 padded.  Either may be NULL. */
int pa_cut_agglo_query(pa_context *ctx, int8_t *agglo_set, int32_t *neighbors);
/* cell tags (element_location per cell) and, for cut cells, their index in the cut-cell batch
 * (-1 otherwise).  Host arrays of ncells entries; either may be NULL.  *ncut may be NULL. */
int pa_cut_query(pa_context *ctx, size_t *ncut, int8_t *cell_location, int32_t *cut_index);
/* The cut cells' local operators (cuthho_square.cpp:308-388, 566-621, 623-666) with
 * hho_degree_info(face_deg + 1, face_deg) (cuthho_square.cpp:871), batched over the ncut cut
 * cells in ascending cell order: d_oper ncut x rbs x msize (cut cells keep the constant mode:
 * rbs rows), d_data/d_stab/d_lc ncut x msize^2, d_rhs ncut x cbs, d_info ncut.  Any may be NULL.
 * `where` = PA_LOC_NEGATIVE or PA_LOC_POSITIVE; rhs_fn / bcs_fn = PA_FN_* built-ins. */
int pa_cut_local_ops_batch(pa_context *ctx, int face_deg, const pa_level_set *ls, int where, int rhs_fn, int bcs_fn,
                           double *d_oper, double *d_data, double *d_stab, double *d_lc, double *d_rhs,
                           int32_t *d_info);
/* Tags and displaced coordinates left by pa_cut_preprocess (host arrays; any may be NULL):
 * node_location npoints (of the UNDISPLACED mesh: detect_node_position is not re-run after
 * move_nodes, cuthho_square.cpp:2036-2049), face_location nfaces, points npoints x 2. */
int pa_cut_query_tags(pa_context *ctx, int8_t *node_location, int8_t *face_location, double *points);
/* Quadrature lists of the cut cells as the cut integrate() overloads produce them
 * (cuthho_geom.hpp:798-815, 851-895), for callers that sample their own functions:
 * which = 0: integrate(msh, cl, 2*recdeg, where); 1: integrate_interface(msh, cl, 2*recdeg, where);
 * 2: integrate_interface(msh, cl, recdeg, where) (the rule cut make_rhs uses, :647).  HOST outputs:
 * h_offsets ncut+1, h_xyw count x 3; pass NULL to query *count. */
int pa_cut_quadrature_points(pa_context *ctx, int face_deg, int where, int which, uint32_t *h_offsets, double *h_xyw,
                             size_t *count);
/* cut make_rhs (:623-666) with caller-sampled functions: d_rhs_vals at the points of list 0,
 * d_bcs_vals at the points of list 2.  d_rhs ncut x cbs. */
int pa_cut_rhs_sampled_batch(pa_context *ctx, int face_deg, const pa_level_set *ls, int where, const double *d_rhs_vals,
                             const double *d_bcs_vals, double *d_rhs);
/* make_rhs(msh, cl, degree, where, f) of the fictitious-domain driver for the UNCUT cells (cuthho_square.cpp:623-631, fan
 * quadrature of degree 2*degree): the cells on the `where` side get utils.hpp:163-171, every other cell -- outside the domain,
 * or cut: pa_cut_merge puts the cut kernel's right-hand side there -- gets zeros without being integrated (at 512 x 512 with
 * the circle of radius 0.35 that is 61 % of the cells).  d_rhs: ncells x cbs(degree); the same values pa_cell_rhs_batch
 * followed by pa_cut_merge's zeroing leaves. */
int pa_cut_uncut_rhs_batch(pa_context *ctx, int degree, int where, int fn, double *d_rhs);
/* Merge for the assembly loop of cuthho_square.cpp:883-900: rows of the cut cells in the
 * cell-major d_lc / d_rhs (all cells, from pa_local_ops_batch(PA_QUAD_FAN, PA_STAB_NAIVE) and
 * pa_cell_rhs_batch) are replaced by the cut operators; the right-hand side of uncut cells
 * outside `where` is zeroed (cuthho_square.cpp:659-664). */
int pa_cut_merge(pa_context *ctx, int face_deg, int where, const double *d_cut_lc, const double *d_cut_rhs,
                 double *d_lc, double *d_rhs);
/* The merge of the condensed mode: the packed records of the cut cells -- pa_static_condensation_packed_batch of their local
 * matrices and right-hand sides (pa_cut_local_ops_batch), d_cut_Sp ncut x nf(nf+1)/2 and d_cut_g ncut x nf -- replace the
 * cut cells' records in d_cond (pa_condensed_ops_batch over all cells with the uncut formulas, n x (nf(nf+1)/2 + nf)). */
int pa_cut_merge_condensed(pa_context *ctx, int face_deg, const double *d_cut_Sp, const double *d_cut_g, double *d_cond);
/* The "Matrix assembly" span of the fictitious-domain driver (apps/cuthho/cuthho_square.cpp:881-905) in one pass: the system is
 * the plain assembler<Mesh>'s over ALL cells (assemble hho.hpp:344-406, finalize hho.hpp:451-455), so the pattern is the one
 * pa_assembler_csr_query / _pattern describe for hho_degree_info(face_deg + 1, face_deg) (cuthho_square.cpp:871) on the same
 * pa_cut_preprocess context.  The uncut cells go through pa_assembler_csr_assemble's pass (PA_QUAD_FAN, PA_STAB_NAIVE,
 * cuthho_square.cpp:316-317, 572-573; in pieces under pa_context_set_record_cap) with the cells tagged PA_LOC_ON_INTERFACE left
 * out of its scatter; their operators -- d_cut_lc, ncut x msize^2 column-major as pa_cut_local_ops_batch writes d_lc, and
 * d_cut_rhs, ncut x cbs or NULL = 0 -- go through the same scatter from a second, small kernel.  No ncells x msize^2 buffer
 * exists unless d_lc asks for one.  A cut kernel still out on the side stream (pa_context_set_cut_overlap) is joined first.
 * d_rhs ncells x cbs or NULL = 0 (pa_cut_uncut_rhs_batch; an uncut cell outside `where` takes a zero right-hand side whatever
 * d_rhs holds there, pa_cut_merge's rule, cuthho_square.cpp:659-664), d_g pa_dirichlet_data_batch or NULL, d_RHS nrows (may be
 * NULL), d_info ncells (may be NULL: the flags of the uncut formulas, for every cell).
 * Contract: d_values and d_RHS are BIT-IDENTICAL to pa_assembler_csr_fill fed with the merged local matrices -- the d_lc this
 * call returns: the assembling instance's image in the uncut rows, a bit copy of d_cut_lc in the cut rows -- the merged
 * right-hand sides (d_rhs with the rule above in the uncut rows, d_cut_rhs in the cut rows) and the same d_g; with or without
 * d_lc, from call to call and whatever the buffers held before.  A face's own diagonal block and right-hand side take one
 * addend per adjacent cell, cut or not; they are added onto entries the call zeroes first, a two-term sum that does not depend
 * on arrival order.  Every other entry is written exactly once.  With no cut cell the result is pa_assembler_csr_assemble's.
 * Refused before any buffer is touched: NULL ctx / d_values, `where` not PA_LOC_NEGATIVE / PA_LOC_POSITIVE, cut cells without
 * d_cut_lc: PA_ERR_INVALID_ARG; no cut preprocessing: PA_ERR_NO_MESH; a slab (pa_cut_preprocess_rows): as pa_assembler_csr_fill;
 * face_deg > 2: PA_ERR_QUADRATURE, as the cut entries. */
int pa_fictdom_csr_assemble(pa_context *ctx, int face_deg, int where,
                            const double *d_rhs, const double *d_g,
                            const double *d_cut_lc, const double *d_cut_rhs,
                            double *d_values, double *d_RHS,
                            double *d_lc /* may be NULL */, int32_t *d_info /* may be NULL */);
/* The same system (assembly loop apps/cuthho/cuthho_square.cpp:881-905, solve :915-919, take_local_data :959-962) condensed to
 * its face unknowns.  It is assembler<Mesh>'s over all cells, so numbering, pattern, fill, halo and expansion are the plain
 * mesh's: pa_condensed_query / _csr_pattern / _csr_fill / _halo_pack / _expand_solution with hho_degree_info(face_deg + 1,
 * face_deg) take the records this call writes.  d_cond: ncells x (nf(nf+1)/2 + nf), pa_condensed_ops_batch's layout
 * (nf = 4 fbs).  An uncut cell's row is the fused condensed pass's (PA_QUAD_FAN, PA_STAB_NAIVE), BIT-IDENTICAL to
 * pa_condensed_ops_batch fed the same right-hand side; an uncut cell outside `where` takes a zero right-hand side whatever
 * d_rhs holds there (pa_fictdom_csr_assemble's rule).  A cut cell's row comes from d_cut_lc / d_cut_rhs
 * (pa_cut_local_ops_batch) by an elimination in double-double -- Cholesky of A_TT, S = A_FF - A_FT A_TT^-1 A_TF and
 * g = -A_FT A_TT^-1 f_T rounded to double once -- because A_TT of a sliver cell has condition numbers to 1e8, which cost the
 * plain-double route (pa_static_condensation_packed_batch + pa_cut_merge_condensed) up to 7 digits.  d_rhs ncells x cbs or
 * NULL = 0; d_cut_rhs ncut x cbs or NULL = 0; d_info ncells (may be NULL: the flags of the uncut formulas, for every cell);
 * d_info_cut ncut (may be NULL): 200 + j + 1 for a failed pivot j of a cut cell's A_TT, else 0.  A cut kernel still out on the
 * side stream (pa_context_set_cut_overlap) is joined first.  Deterministic call to call.  A slab context
 * (pa_cut_preprocess_rows) is accepted: the work is cell-local.
 * Refused before any buffer is touched, in pa_fictdom_csr_assemble's order: NULL ctx / d_cond, `where` not PA_LOC_NEGATIVE /
 * PA_LOC_POSITIVE: PA_ERR_INVALID_ARG; no cut preprocessing: PA_ERR_NO_MESH; face_deg > 2: PA_ERR_QUADRATURE; cut cells without
 * d_cut_lc: PA_ERR_INVALID_ARG. */
int pa_fictdom_condensed_ops_batch(pa_context *ctx, int face_deg, int where,
                                   const double *d_rhs, const double *d_cut_lc, const double *d_cut_rhs,
                                   double *d_cond, int32_t *d_info /* may be NULL */, int32_t *d_info_cut /* may be NULL */);
/* The cell unknowns of that system from its face solution (apps/cuthho/cuthho_square.cpp:881-905 assembled it, :915-919 solved
 * it, :959-962 take_local_data reads it): u_T = A_TT^-1 (f_T - A_TF u_F) for every cell of the context.  Uncut cells: the pass
 * of pa_condensed_recover_batch on the face values of pa_condensed_take_faces, bit-identical to those calls; cut cells: in
 * double-double from d_cut_lc / d_cut_rhs.  u_F of a Dirichlet face is d_g (NULL = 0) for cut and uncut cells alike -- the plain
 * assembler's rule; a cut cell on the boundary occurs with the line level set.  d_xF: the face solution (system_size of
 * pa_condensed_query); d_full: the reference's full solution vector, cbs ncells_global + system_size, cells first -- the
 * context's own cells (a slab: its rows, as pa_condensed_expand_solution) and a bit copy of d_xF behind the cells.  d_rhs,
 * d_cut_lc, d_cut_rhs, `where`, the side stream and the refusals as pa_fictdom_condensed_ops_batch (d_full in place of d_cond;
 * NULL d_xF: PA_ERR_INVALID_ARG). */
int pa_fictdom_condensed_recover(pa_context *ctx, int face_deg, int where,
                                 const double *d_rhs, const double *d_cut_lc, const double *d_cut_rhs,
                                 const double *d_g, const double *d_xF, double *d_full);

/* ---- cutHHO two-sided interface problem (`cuthho_square -i`, run_cuthho_interface
 * cuthho_square.cpp:1625-1846).  hho_degree_info(face_deg + 1, face_deg) (:1662). */
typedef struct { double kappa_1, kappa_2, eta; } pa_interface_params;      /* params<T> :293-299: 1, 1, 5 */
/* Cut cells, in ascending cell order.  Unknowns of a cut cell: [cell-, cell+, faces-, faces+]
 * (2*msize).  d_oper ncut x (2rbs x 2msize) and d_data ncut x (2msize)^2: make_hho_laplacian_interface
 * (:390-502); gr_lhs is semi-definite (the reference uses Eigen's pivoted LDLT): `oper` comes back
 * with the constant of the negative side pinned to zero, `data` does not depend on that choice.
 * d_lc ncut x (2msize)^2: data + kappa_1 * make_hho_cut_stabilization(NEGATIVE) + kappa_2 * (POSITIVE)
 * scattered as :1694-1705.  d_rhs ncut x 2cbs: make_rhs(msh, cl, degree, where, f) of both sides
 * (cuthho_utils.hpp:65-84, :1710-1711).  Any output may be NULL. */
int pa_cut_interface_ops_batch(pa_context *ctx, int face_deg, const pa_level_set *ls, const pa_interface_params *parms,
                               int rhs_fn, double *d_oper, double *d_data, double *d_lc, double *d_rhs, int32_t *d_info);
/* Uncut cells (:1668-1681): d_lc ncells x msize^2 = kappa(side) * make_hho_laplacian.second +
 * make_hho_naive_stabilization (fan quadrature), d_rhs ncells x cbs = make_rhs(f).  Rows of cut
 * cells hold the uncut formulas too and are ignored by pa_interface_triplets_batch. */
int pa_cut_interface_uncut_batch(pa_context *ctx, int face_deg, const pa_interface_params *parms, int rhs_fn,
                                 double *d_lc, double *d_rhs, int32_t *d_info);
/* interface_assembler (:1091-1443): sizes of the system with duplicated unknowns */
typedef struct {
    uint64_t num_all_cells;      /* cell blocks, cut cells counted twice              :1142-1150 */
    uint64_t num_other_faces;    /* non-Dirichlet face blocks, cut faces counted twice :1152-1163 */
    uint64_t system_size;        /* cbs * num_all_cells + fbs * num_other_faces        :1185      */
    uint64_t ncut;
} pa_interface_info;
int pa_interface_assembler_query(pa_context *ctx, int face_deg, pa_interface_info *out);
/* interface_assembler::assemble (:1203-1269) for the uncut cells and assemble_cut (:1271-1354)
 * for the cut cells.  Uncut: d_rows/d_cols/d_vals ncells x msize^2 (slot i*msize + j; -1 for
 * dropped slots and for every slot of a cut cell), d_rhs_rows/d_rhs_vals ncells x msize.  Cut:
 * d_rows_cut/... ncut x (2msize)^2, d_rhs_rows_cut/d_rhs_vals_cut ncut x 2msize.  d_g: Dirichlet
 * data (pa_dirichlet_data_batch) or NULL. */
int pa_interface_triplets_batch(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_g,
                                const double *d_lc_cut, const double *d_rhs_cut,
                                int32_t *d_rows, int32_t *d_cols, double *d_vals,
                                int32_t *d_rows_cut, int32_t *d_cols_cut, double *d_vals_cut,
                                int32_t *d_rhs_rows, double *d_rhs_vals, int32_t *d_rhs_rows_cut, double *d_rhs_vals_cut);
/* cell dofs read back by interface_assembler::take_local_data (:1356-1379): d_offsets ncells x 2 =
 * offset in the solution of the cell block of the negative / positive side (equal for uncut cells) */
int pa_interface_cell_offsets(pa_context *ctx, int face_deg, int64_t *d_offsets);
/* The same system -- what assemble / assemble_cut (:1203-1354) + finalize = setFromTriplets (:1437-1441) leave in `LHS` /
 * `RHS` -- built DIRECTLY in CSR from the tables of pa_cut_preprocess: no triplets, no sort.  With pa_cut_interface_uncut_batch,
 * pa_cut_interface_ops_batch and pa_conjugated_gradient it is the loop of run_cuthho_interface (:1664-1716) and its solve
 * (:1737-1743) on the device.  Symbolic phase, once per cut mesh and face degree (kept by the context, rebuilt by the next
 * pa_cut_preprocess or another face_deg): nrows = system_size, nnz; d_rowptr nrows + 1 (int64), d_colind nnz (int32,
 * ascending within a row; may be NULL).  Numeric phase, once per assembly: d_values nnz and d_RHS nrows (may be NULL) from
 * d_lc / d_rhs (ncells x msize^2 / ncells x cbs, pa_cut_interface_uncut_batch; rows of cut cells unused; d_rhs may be NULL),
 * d_g (pa_dirichlet_data_batch or NULL) and d_lc_cut / d_rhs_cut (ncut x (2msize)^2 / ncut x 2cbs,
 * pa_cut_interface_ops_batch; d_rhs_cut may be NULL).  Local matrices column-major.  Structure and values bit-identical to
 * pa_csr_from_triplets of pa_interface_triplets_batch's slots taken in cell order (a cut cell's block in place of its
 * uncut one); d_RHS the scatter-add of its d_rhs_vals / d_rhs_vals_cut in the same order.  Refuses what
 * pa_interface_triplets_batch refuses (face_deg 0..3, whole-mesh cut contexts, system_size < 2^31, d_lc_cut when ncut > 0);
 * joins pending side-stream work (pa_context_set_cut_overlap) first. */
int pa_interface_csr_query(pa_context *ctx, int face_deg, pa_assembler_csr_info *out);
int pa_interface_csr_pattern(pa_context *ctx, int face_deg, int64_t *d_rowptr, int32_t *d_colind);
int pa_interface_csr_fill(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_g,
                          const double *d_lc_cut, const double *d_rhs_cut, double *d_values, double *d_RHS);
/* The same system after static condensation: the cell unknowns of every cell eliminated (each couples only inside its cell), the
 * face unknowns left in interface_assembler's numbering without its cell blocks -- unknown k of face block b at
 * (face_table[F] + b) * fbs + k (:1152-1185), system_size = fbs * num_other_faces.  nf = 4 fbs face unknowns per uncut cell,
 * NF = 8 fbs per cut cell ([faces-, faces+] of pa_cut_interface_ops_batch).  Stands in for the assembly loop (:1664-1716), the
 * solve (:1737-1743) and the cell part of take_local_data (:1356-1379): the face-only system goes to pa_conjugated_gradient,
 * pa_interface_condensed_recover gives back the full solution vector.
 *   _query: system_size, nnz, nf, NF and the doubles per uncut / cut record.
 *   _ops_batch: records from the inputs of pa_interface_csr_fill.  d_cond ncells x cond_doubles laid out as [S of every cell |
 *     g of every cell] (S the upper triangle of A_FF - A_FT A_TT^-1 A_TF, column-packed, nf(nf+1)/2; g = -A_FT A_TT^-1 f_T),
 *     bit-identical to pa_static_condensation_packed_batch of d_lc / d_rhs (rows of cut cells computed, never read); d_cond_cut
 *     ncut x cond_cut_doubles the same for the cut cells, computed in double-double (the cut cells' A_TT has condition numbers
 *     to 1e8) and rounded once.  d_info (ncells) / d_info_cut (ncut), may be NULL: 200 + j + 1 for a failed pivot j, else 0.
 *   _triplets_batch: the assembly of the records as triplets in the reference's push order (cells ascending, local row, local
 *     column): d_rows / d_cols / d_vals ncells x nf^2 (cut cells: all -1), *_cut ncut x NF^2, d_rhs_rows / d_rhs_vals ncells x nf,
 *     *_cut ncut x NF.  Dirichlet columns of uncut cells go to the right-hand side with d_g (g_i - sum_j S_ij u_D,j, as
 *     pa_condensed_triplets_batch); a cut cell's slots on a Dirichlet face are dropped (pa_interface_triplets_batch).
 *   _csr_pattern / _csr_fill: the same matrix directly in CSR (d_rowptr system_size + 1, d_colind nnz may be NULL; d_values nnz,
 *     d_rhs system_size may be NULL), bit-identical to pa_csr_from_triplets of the triplets taken in cell order.  It is the
 *     face-face block of pa_interface_csr_pattern with column ids shifted by cbs * num_all_cells.
 *   _recover: u_T = A_TT^-1 (f_T - A_TF u_F) of every cell (cut cells in double-double) from the face-only solution d_xF and the
 *     inputs of _ops_batch; d_full (pa_interface_assembler_query's system_size) is the full solution vector in the reference's
 *     numbering: cell blocks at cell_table offsets, then d_xF -- what take_local_data and pa_interface_cell_offsets read.  u_F of
 *     a Dirichlet face is d_g for an uncut cell, zero for a cut cell (its slots were dropped).
 * All refuse what pa_interface_csr_* refuses, in its order (face_deg 0..3, whole-mesh cut contexts, system_size < 2^31, the
 * cut-cell arrays when ncut > 0), and join pending side-stream work (pa_context_set_cut_overlap) first. */
typedef struct {
    uint64_t system_size, nnz;
    int32_t nf, NF;                              /* face unknowns of an uncut / cut cell */
    int32_t cond_doubles, cond_cut_doubles;      /* doubles per uncut / cut record */
} pa_interface_condensed_info;
int pa_interface_condensed_query(pa_context *ctx, int face_deg, pa_interface_condensed_info *out);
int pa_interface_condensed_ops_batch(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_lc_cut,
                                     const double *d_rhs_cut, double *d_cond, double *d_cond_cut, int32_t *d_info, int32_t *d_info_cut);
int pa_interface_condensed_triplets_batch(pa_context *ctx, int face_deg, const double *d_cond, const double *d_cond_cut, const double *d_g,
                                          int32_t *d_rows, int32_t *d_cols, double *d_vals, int32_t *d_rows_cut, int32_t *d_cols_cut,
                                          double *d_vals_cut, int32_t *d_rhs_rows, double *d_rhs_vals, int32_t *d_rhs_rows_cut,
                                          double *d_rhs_vals_cut);
int pa_interface_condensed_csr_pattern(pa_context *ctx, int face_deg, int64_t *d_rowptr, int32_t *d_colind);
int pa_interface_condensed_csr_fill(pa_context *ctx, int face_deg, const double *d_cond, const double *d_cond_cut, const double *d_g,
                                    double *d_values, double *d_rhs);
int pa_interface_condensed_recover(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_lc_cut,
                                   const double *d_rhs_cut, const double *d_g, const double *d_xF, double *d_full);
/* The patch tables of that face-only system for pa_patch_precond_* / pa_conjugated_gradient_patch (solver_cg.hpp:63-144 with
 * patches where the reference has 1 / diag(A); the solve they serve is cuthho_square.cpp:1737-1743), in interface_assembler's
 * numbering, in which a cut face owns two blocks: rows are rows of pa_interface_condensed_csr_pattern, `kind` is that of
 * pa_condensed_patches, the table format that of pa_patch_precond_*.
 *   PA_PATCH_FACE: one patch per non-Dirichlet face by ascending face id: all rows of its blocks, fbs for an uncut face, 2 fbs
 *     for a cut face (negative block, then positive block); at most 8 rows.  The patches partition the rows in order.  (A cut
 *     face on the Dirichlet boundary -- a level set that leaves the domain, which interface_assembler refuses -- is counted by
 *     pa_cut_preprocess's numbering and owns nothing: its empty row group lies in no patch of either kind.)
 *   PA_PATCH_CELL: by ascending cell id.  An uncut cell with a non-Dirichlet face gives one patch: the blocks of its
 *     non-Dirichlet faces in the cell's face order bottom, right, top, left.  A cut cell gives up to two, negative side first:
 *     the patch of a side holds, in that order, of a cut face the side's block, of an uncut face its one block only if the face
 *     lies on that side.  Dirichlet faces are skipped, a side without rows gives no patch; at most 4 fbs <= PA_PATCH_MAX_ROWS
 *     rows.  Every block of an interior face lies in exactly two cell patches.
 * The query gives the sizes of d_patch_ptr (*npatches + 1) and d_patch_rows (*entries).  Refused, before anything is written:
 * what pa_interface_csr_* refuses, in its order (face_deg 0..3, whole-mesh cut contexts, system_size < 2^31); an unknown kind or
 * a NULL output (PA_ERR_INVALID_ARG); a table of 2^31 entries or more.  Pending side-stream work (pa_context_set_cut_overlap)
 * is joined first.  Both wait for the stream. */
int pa_interface_condensed_patches_query(pa_context *ctx, int face_deg, int kind, size_t *npatches, size_t *entries);
int pa_interface_condensed_patches(pa_context *ctx, int face_deg, int kind, int64_t *d_patch_ptr, int32_t *d_patch_rows);
/* The coarse table of that face-only system for pa_coarse_precond_* / pa_conjugated_gradient_patch_coarse (solver_cg.hpp:63-144
 * with z = patch sum + P (P^T A P)^-1 P^T r where the reference has 1 / diag(A); the solve it serves is
 * cuthho_square.cpp:1737-1743), in interface_assembler's numbering, built on the device.  Rows are rows of
 * pa_interface_condensed_csr_pattern: unknown k of block b at b fbs + k; an uncut non-Dirichlet face owns one block, a cut face
 * two (negative side, then positive side).  The hats are pa_condensed_coarse's -- the same coarse lines, 1-D and 2-D hats and
 * node order, the same arithmetic -- and so are the entries of a block: from the end points a, b of its face, row b fbs gets
 * 0.5 * (phi(a) + phi(b)) for every node with phi(a) != 0 or phi(b) != 0, row b fbs + 1 (fbs >= 2) gets 0.5 * (phi(b) - phi(a))
 * where that is not zero, higher modes are empty.  The face basis of a cut face is the whole face's (cuthho_square.cpp:371, 471,
 * 594): both of its blocks get the same values.
 *   PA_COARSE_ONE: the column is the node.  PA_COARSE_BY_SIDE: the block of an uncut face is in the part of the face's side
 *   (0 negative, 1 positive), a cut face's first block in part 0 and its second in part 1; part-0 columns come first, then the
 *   part-1 columns, each in node order; columns no block touches are dropped -- the table pa_condensed_coarse(..,
 *   PA_COARSE_BY_SIDE, PA_LOC_NEGATIVE) would build if every block were a face of its own.
 * A cut face on the Dirichlet boundary is counted by the numbering and owns nothing: its row group stays empty (equal pointers).
 * The query gives ncoarse and the size of d_p_cols / d_p_vals (*entries); d_p_ptr takes system_size + 1.  Refused, before
 * anything is written: what pa_interface_csr_* refuses, in its order (face_deg 0..3, whole-mesh cut contexts, system_size <
 * 2^31); H < 1, an unknown `parts` or a NULL output (PA_ERR_INVALID_ARG); no interior node, or more than PA_COARSE_MAX_NODES
 * columns (PA_ERR_INVALID_ARG with H and the count in pa_last_error()).  Pending side-stream work
 * (pa_context_set_cut_overlap) is joined first.  Both wait for the stream. */
int pa_interface_condensed_coarse_query(pa_context *ctx, int face_deg, int H, int parts, size_t *ncoarse, size_t *entries);
int pa_interface_condensed_coarse(pa_context *ctx, int face_deg, int H, int parts, int64_t *d_p_ptr, int32_t *d_p_cols,
                                  double *d_p_vals);

/* The face-only system of interface_assembler assembled and solved BY ROW SLABS (cuthho_square.cpp:1142-1178 the numbering,
 * :1203-1354 the assembly, :1664-1743 the loop and the solve; the reference has one process).  The context is one of
 * pa_cut_preprocess_rows -- rank r holds cell rows [row_begin, row_end) -- or of pa_cut_preprocess, the one-slab case.  Every rank
 * runs the same whole-mesh host preprocessing, so the first block of any cell or face is a prefix count it can take itself (:1142-1163);
 * no table moves between ranks.  Faces are ordered by (low point, high point): the faces whose low point lies in the slab's node
 * rows -- the bottom and vertical faces of its cell rows -- are one contiguous range of face blocks, the OWNED rows
 * [row_begin, row_end) of the system.  An owned bottom face takes addends from the cell below it, on the rank below: the one thing a
 * step moves is the records of a slab's top cell row, one slab up (pa_comm_halo_exchange_start).  The slabs' rows stacked are
 * pa_interface_condensed_csr_*'s system of the whole mesh BIT FOR BIT; so are the records and the recovered cell unknowns.
 *   _partition_info: the info of a slab from the mesh parameters alone: host only, no context, no device.
 *   _query: the same from the context (nnz_owned from its symbolic tables).
 *   _ops_batch: pa_interface_condensed_ops_batch on the slab's cells: d_cond ncells x cond_doubles [S of every cell | g of every
 *     cell], d_cond_cut ncut x cond_cut_doubles, of the outputs of pa_cut_interface_uncut_batch / pa_cut_interface_ops_batch on
 *     the slab; the info conventions unchanged.
 *   _halo_pack: what the slab above needs, halo_send_doubles doubles into d_halo, ordered on the context's stream: [S of the top
 *     row's halo_send_cells cells | their g | S of its halo_send_cut cut cells | their g | halo_send_cells x nf boundary values:
 *     d_g of each cell's four faces in local order, zero where a face is not Dirichlet (d_g NULL: all zero)].  Nothing on the top
 *     slab.  d_g is indexed by the context's own faces (pa_dirichlet_data_batch on the slab).
 *   _csr_pattern / _csr_fill: the owned rows in CSR: d_rowptr nrows_owned + 1 LOCAL (starts at 0), d_colind nnz_owned GLOBAL column
 *     ids of the face-only system, ascending within a row (may be NULL) -- the form pa_conjugated_gradient_rows takes; d_values
 *     nnz_owned; d_rhs nrows_owned (may be NULL).  d_halo_below: the _halo_pack output of the slab below (NULL on slab 0).  The
 *     Dirichlet columns of an uncut cell go to the right-hand side (g_i - sum_j S_ij u_D,j), a halo cell's with the boundary values
 *     of the halo: the same sum of the same numbers as on the whole mesh.
 *   _recover: u_T = A_TT^-1 (f_T - A_TF u_F) of the slab's cells (pa_interface_condensed_recover's arithmetic).  d_xF: the face
 *     solution over [row_begin, col_end), its tail beyond row_end received from the rank above
 *     (pa_comm_neighbour_exchange_start); d_uT: the slab's cell blocks [cell_block_begin, cell_block_end), cbs doubles each,
 *     contiguous in the full numbering.
 * The refusals, in this order: face_deg outside 0..3 (PA_ERR_INVALID_DEGREE); no cut mesh (PA_ERR_NO_MESH); system_size >= 2^31;
 * the cut-cell arrays missing while the slab has cut cells; d_halo_below missing while the slab has a row below.  Pending
 * side-stream work (pa_context_set_cut_overlap) is joined first.  The pa_interface_* entry points above keep refusing a slab. */
typedef struct {
    uint64_t system_size;                        /* of the whole mesh's face-only system */
    uint64_t row_begin, row_end, nnz_owned;      /* the owned rows and their entries */
    uint64_t col_begin, col_end;                 /* the columns the owned rows read; _recover reads [row_begin, col_end) */
    uint64_t cell_block_begin, cell_block_end;   /* the slab's cell blocks in interface_assembler's full numbering */
    int32_t nf, NF;                              /* face unknowns of an uncut / cut cell */
    int32_t cond_doubles, cond_cut_doubles;      /* doubles per uncut / cut record */
    uint64_t halo_send_cells, halo_send_cut, halo_send_doubles;     /* sent up: 0 on the top slab */
    uint64_t halo_recv_cells, halo_recv_cut, halo_recv_doubles;     /* received from below: 0 on slab 0 */
} pa_interface_rows_info;
int pa_interface_rows_partition_info(size_t Nx, size_t Ny, double min_x, double max_x, double min_y, double max_y, const pa_level_set *ls,
                                     int refsteps, size_t row_begin, size_t row_end, int face_deg, pa_interface_rows_info *out);
int pa_interface_rows_query(pa_context *ctx, int face_deg, pa_interface_rows_info *out);
int pa_interface_rows_ops_batch(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_lc_cut,
                                const double *d_rhs_cut, double *d_cond, double *d_cond_cut, int32_t *d_info, int32_t *d_info_cut);
int pa_interface_rows_halo_pack(pa_context *ctx, int face_deg, const double *d_cond, const double *d_cond_cut, const double *d_g,
                                double *d_halo);
int pa_interface_rows_csr_pattern(pa_context *ctx, int face_deg, int64_t *d_rowptr, int32_t *d_colind);
int pa_interface_rows_csr_fill(pa_context *ctx, int face_deg, const double *d_cond, const double *d_cond_cut, const double *d_g,
                               const double *d_halo_below, double *d_values, double *d_rhs);
int pa_interface_rows_recover(pa_context *ctx, int face_deg, const double *d_lc, const double *d_rhs, const double *d_lc_cut,
                              const double *d_rhs_cut, const double *d_g, const double *d_xF, double *d_uT);
/* The tables of ONE SLAB of that system for pa_conjugated_gradient_rows_patch_coarse (solver_cg.hpp:63-144 with z = patch sum +
 * P (P^T A P)^-1 P^T r where the reference has 1 / diag(A); the solve they serve is cuthho_square.cpp:1737-1743), in
 * interface_assembler's numbering (cuthho_square.cpp:1142-1178), in which a cut face owns two blocks, built on the device from
 * the slab's own tables.  The context is one of pa_cut_preprocess_rows -- the owned rows [row_begin, row_end) of
 * pa_interface_rows_query -- or of pa_cut_preprocess, the one-slab case, which gives pa_interface_condensed_patches' /
 * pa_interface_condensed_coarse's tables exactly.  The formats are those of pa_patch_precond_* / pa_coarse_precond_*; rows are
 * GLOBAL indices of the face-only system.  No operators, no halo and no communication are needed.
 *   Patches, in terms of pa_interface_condensed_patches' whole-mesh table.  PA_PATCH_FACE: its patches whose rows lie in
 *   [row_begin, row_end), in order, d_patch_ptr rebased to 0; both blocks of a cut face are owned together, so the slabs' tables
 *   concatenated are the whole-mesh table.  PA_PATCH_CELL: its patches of the slab's OWN cells (never the halo row's), one per
 *   uncut cell and one per side of a cut cell, negative side first, by ascending cell id, with every row outside [row_begin,
 *   row_end) deleted and a patch that keeps no row dropped: a cell of the top row of a slab that is not the last loses its top
 *   face, both blocks of it if it is cut.  Every row lies within the range and every owned row that exists in at least one patch;
 *   the empty row group of a cut face on the Dirichlet boundary lies in none.
 *   Coarse: rows [row_begin, row_end) of pa_interface_condensed_coarse's whole-mesh table BIT FOR BIT -- the same hats on the
 *   whole mesh's vertex indices, the same arithmetic --, the same ncoarse and column ids on every rank, d_p_ptr (row_end -
 *   row_begin + 1) from 0.  PA_COARSE_ONE and PA_COARSE_BY_SIDE; by side the columns no block touches are dropped as the WHOLE
 *   mesh decides, from the tags every rank's own preprocessing holds, not from the slab's blocks.
 * The queries give the sizes as their whole-mesh siblings do.  Refused, before anything is written: what pa_interface_rows_*
 * refuses, in its order (nothing here needs the cut-cell arrays or a halo); an unknown kind / parts, H < 1 or a NULL output
 * (PA_ERR_INVALID_ARG); no interior node, or more than PA_COARSE_MAX_NODES columns (H and the count in pa_last_error()); a table
 * of 2^31 entries or more (a coarse table of 2^29 owned rows or more).  Pending side-stream work (pa_context_set_cut_overlap) is
 * joined first.  All four wait for the stream; no atomics: two calls give the same bits. */
int pa_interface_rows_patches_query(pa_context *ctx, int face_deg, int kind, size_t *npatches, size_t *entries);
int pa_interface_rows_patches(pa_context *ctx, int face_deg, int kind, int64_t *d_patch_ptr, int32_t *d_patch_rows);
int pa_interface_rows_coarse_query(pa_context *ctx, int face_deg, int H, int parts, size_t *ncoarse, size_t *entries);
int pa_interface_rows_coarse(pa_context *ctx, int face_deg, int H, int parts, int64_t *d_p_ptr, int32_t *d_p_cols, double *d_p_vals);

/* ---- multi-GPU exchange: one process per GPU, RCCL over xGMI ------------
 * The reference is a single process without any communication.  Cells shard by rows (pa_mesh_generate's
 * row_begin / row_end); every rank assembles the CSR rows of the faces it owns (pa_condensed_csr_fill), and the only
 * data a step moves between ranks are the packed top-face rows of a slab's top cell row (pa_condensed_halo_pack),
 * one slab up: rank r -> rank r + 1, halo_cells x halo_doubles doubles.  RCCL is bound at run time (dlopen; a copy
 * the process already holds, e.g. PyTorch's, is used), so the library loads without it.
 * Bootstrap as with NCCL: rank 0 calls pa_comm_unique_id and hands the PA_COMM_ID_BYTES to the other ranks (MPI,
 * a file, torch.distributed's store ...); every rank then calls pa_comm_create with its context.
 * The *_start calls are ordered after everything already enqueued on the context's stream and run on a stream of the
 * communicator, next to whatever the context enqueues afterwards; pa_comm_wait orders the context's stream behind
 * them.  Ranks in slab order: rank r owns the cell rows below those of rank r + 1. */
#define PA_COMM_ID_BYTES 128
typedef struct pa_comm pa_comm;
int pa_comm_unique_id(void *id_out, size_t bytes);
int pa_comm_create(pa_context *ctx, int nranks, int rank, const void *unique_id, pa_comm **out);
int pa_comm_destroy(pa_comm *comm);
int pa_comm_info(pa_comm *comm, int *nranks, int *rank);
const char *pa_comm_last_error(pa_comm *comm);
/* d_send_up: this rank's pa_condensed_halo_pack output (ignored on the last rank); d_recv_below: where the rows of
 * the rank below land (ignored on rank 0); counts in doubles */
int pa_comm_halo_exchange_start(pa_comm *comm, const double *d_send_up, size_t send_count,
                                double *d_recv_below, size_t recv_count);
/* every rank's bytes_per_rank bytes to every rank, in rank order (the north star's all-gather of the face-dof
 * blocks, for a caller that wants the whole system on one device) */
int pa_comm_allgather_start(pa_comm *comm, const void *d_send, void *d_recv, size_t bytes_per_rank);
/* in-place sum over the ranks (the dot products of a distributed solve) */
int pa_comm_allreduce_sum_start(pa_comm *comm, double *d_buf, size_t count);
int pa_comm_wait(pa_comm *comm);
/* both neighbours at once (the halo of a vector in a row-partitioned solve): my first n_send_lo doubles to rank - 1, my last
 * n_send_hi to rank + 1; rank - 1's message into d_recv_lo, rank + 1's into d_recv_hi.  Counts of a missing neighbour are
 * ignored. */
int pa_comm_neighbour_exchange_start(pa_comm *comm, const double *d_send_lo, size_t n_send_lo, const double *d_send_hi, size_t n_send_hi,
                                     double *d_recv_lo, size_t n_recv_lo, double *d_recv_hi, size_t n_recv_hi);

/* ---- the reference's conjugated_gradient on a ROW-PARTITIONED system -------------------------------------------
 * (solver_cg.hpp:45-144 has one process; this is the solve of the face-only condensed system where it was assembled:
 * every rank holds the CSR rows [row_begin, row_end) it owns, pa_condensed_csr_fill, with GLOBAL column indices.)
 * Same recurrences and exit tests in the same order as pa_conjugated_gradient; the dot products are local partial sums
 * added over the ranks, the search direction's entries a rank's rows read beyond its own range -- the matrix is symmetric
 * and banded by the mesh's row structure, so they belong to ranks r - 1 and r + 1 -- are refreshed once per iteration.
 * The transport is three callbacks; NULL = one rank (then the call equals pa_conjugated_gradient, bit for bit).
 *   allreduce_sum:    sum of n host doubles over the ranks, in place, the same bits on every rank;
 *   halo:             one neighbour exchange of device ranges (pa_comm_neighbour_exchange_start's arguments; complete or
 *                     ordered on `stream` when it returns);
 *   neighbour_counts: at setup, tell the neighbours how many of their entries this rank reads (need_lo below, need_hi
 *                     above) and learn how many of this rank's first / last entries they read (give_lo, give_hi).
 * Callbacks return 0 on success.  d_b, d_x: the rank's own rows (row_end - row_begin doubles); x starts from zero.
 * *transport_status: 0 ok, 1 a callback failed on this rank, 2 this rank's rows read beyond what the neighbours can give (or,
 * without a transport, beyond the own range), 3 ANOTHER rank failed, 4 a HIP error on this rank.  Every exit is collective: a
 * rank's local failure rides as a flag on the next all-reduce (one extra addend: allreduce_sum is called with up to 3 values)
 * and all ranks return from the same reduction -- PA_ERR_COMM (1, 3), PA_ERR_INVALID_ARG (2), PA_ERR_HIP (4) --, none is left
 * inside a collective or a neighbour exchange. */
typedef struct {
    void *user;
    int (*allreduce_sum)(void *user, double *vals, int n);
    int (*halo)(void *user, const double *d_send_lo, size_t n_send_lo, const double *d_send_hi, size_t n_send_hi,
                double *d_recv_lo, size_t n_recv_lo, double *d_recv_hi, size_t n_recv_hi, void *stream);
    int (*neighbour_counts)(void *user, int64_t need_lo, int64_t need_hi, int64_t *give_lo, int64_t *give_hi);
} pa_cg_transport;
int pa_conjugated_gradient_rows(pa_context *ctx, const pa_cg_transport *transport, int64_t row_begin, int64_t row_end,
                                const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values, const double *d_b, double *d_x,
                                double convergence_threshold, double divergence_threshold, size_t max_iter, int apply_preconditioner,
                                int32_t *exit_reason, size_t *iterations, double *relative_residual, int32_t *transport_status);
/* plain copies ordered on the context's stream and complete on return (what a host-staged transport needs) */
int pa_copy_to_host(pa_context *ctx, void *host_dst, const void *d_src, size_t bytes);
int pa_copy_to_device(pa_context *ctx, void *d_dst, const void *host_src, size_t bytes);
/* the RCCL transport of a communicator (user = the communicator) */
int pa_comm_cg_transport(pa_comm *comm, pa_cg_transport *out);

/* ---- the patches and the coarse level on the ROW-PARTITIONED system ------------------------------------------
 * pa_conjugated_gradient_rows (solver_cg.hpp:45-144; the solve of cuthho_square.cpp:915-919 where it was assembled) with the
 * preconditioner of pa_conjugated_gradient_patch_coarse, z = (patch sum) + (coarse term), in place of the point Jacobi: the
 * arguments of pa_conjugated_gradient_rows without apply_preconditioner, plus two caller-owned device tables of THIS rank.
 *   Patches: npatches, d_patch_ptr, d_patch_rows as pa_patch_precond_*, the rows GLOBAL indices, every one within [row_begin,
 *   row_end), every owned row in at least one patch.  A patch's block then lies inside the rank's rows and their own columns:
 *   the patch level needs no communication.
 *   Coarse: ncoarse (the same on every rank; 0 = patches only, the three pointers may be NULL), and the rank's own rows of P:
 *   d_p_ptr (row_end - row_begin + 1, from 0), d_p_cols (global coarse columns), d_p_vals, as pa_coarse_precond_*.
 * Set-up: the rows of P for the two ends of the window travel through `halo` (8 doubles a row: four (column as double, value)
 * pairs padded with column -1, so 8 x give sent and 8 x need received), W = A_r P_window, the rank's addend P_r^T W in the
 * one-rank product's fixed order, the lower triangle of A_c through allreduce_sum (in pieces of at most 2^20 + 1 values) and
 * mirrored -- exactly symmetric, the same bits on every rank --, and every rank factors it.
 * Iteration: the recurrences, exit tests and exit order of pa_conjugated_gradient_patch_coarse with three sums over the ranks:
 * d . y; the coarse restriction P_r^T r (ncoarse + 1 values); (r . r, r . z).  No floating-point atomics: two calls with the
 * same inputs give the same bits.  With transport = NULL, row_begin = 0 and whole tables the call is
 * pa_conjugated_gradient_patch_coarse bit for bit, with ncoarse = 0 pa_conjugated_gradient_patch.
 * *transport_status as pa_conjugated_gradient_rows, and 5: a table of this rank was refused (PA_ERR_INVALID_ARG, text in
 * pa_last_error), 6: a patch of this rank or the coarse matrix is not positive definite (PA_ERR_NOT_SPD; a pivot of A_c is the
 * same on every rank, all report 6).  The other ranks leave with 3 and PA_ERR_COMM, all before the first iteration.  d_x is
 * written only when the call returns PA_OK. */
int pa_conjugated_gradient_rows_patch_coarse(pa_context *ctx, const pa_cg_transport *transport, int64_t row_begin, int64_t row_end,
                                             const int64_t *d_rowptr, const int32_t *d_colind, const double *d_values, const double *d_b,
                                             double *d_x, size_t npatches, const int64_t *d_patch_ptr, const int32_t *d_patch_rows,
                                             size_t ncoarse, const int64_t *d_p_ptr, const int32_t *d_p_cols, const double *d_p_vals,
                                             double convergence_threshold, double divergence_threshold, size_t max_iter,
                                             int32_t *exit_reason, size_t *iterations, double *relative_residual, int32_t *transport_status);
/* The tables of a slab for that call (assembler::assemble hho.hpp:344-406 numbers the faces; a context of pa_mesh_generate(..,
 * row_begin, row_end), the whole mesh being the slab of all rows), built on the device from the mesh's closed forms.
 *   Patches, rows as GLOBAL indices.  PA_PATCH_FACE: one patch per owned non-Dirichlet face.  PA_PATCH_CELL: one patch per cell of
 *   the slab with an owned non-Dirichlet face, the rows of those faces in the order bottom, right, top, left; a cell of the top
 *   row of a slab that is not the last loses its top face, which the slab above owns.  The face tables of the slabs, concatenated,
 *   are pa_condensed_patches' of the whole mesh; the cell tables are its table with every row outside the patch's slab deleted.
 *   Coarse (basic_mesh.hpp:230-298 gives the vertex indices the hats live on), PA_COARSE_ONE only: rows [row_begin, row_end) of
 *   pa_condensed_coarse's whole-mesh table bit for bit, the same ncoarse and column ids, d_p_ptr rebased to 0.
 * Not served: PA_COARSE_BY_SIDE (PA_ERR_INVALID_ARG), the single-process C++ headers; the slabs of the interface problem have
 * pa_interface_rows_patches / pa_interface_rows_coarse, and the solver above takes any caller's table.  Other refusals as
 * pa_condensed_patches / pa_condensed_coarse. */
int pa_condensed_rows_patches_query(pa_context *ctx, pa_degree_info di, int kind, size_t *npatches, size_t *entries);
int pa_condensed_rows_patches(pa_context *ctx, pa_degree_info di, int kind, int64_t *d_patch_ptr, int32_t *d_patch_rows);
int pa_condensed_rows_coarse_query(pa_context *ctx, pa_degree_info di, int H, int parts, size_t *ncoarse, size_t *entries);
int pa_condensed_rows_coarse(pa_context *ctx, pa_degree_info di, int H, int parts, int64_t *d_p_ptr, int32_t *d_p_cols, double *d_p_vals);

/* occupancy / launch facts of the dominant kernel for the roofline bookkeeping */
typedef struct {
    int32_t lanes_per_cell, cells_per_block, block_threads, lds_bytes_per_block;
    int32_t grid_blocks;
    const char *kernel_name;
} pa_launch_info;
int pa_local_ops_launch_info(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind,
                             size_t n, pa_launch_info *out);
/* the same for the condensed-mode instance (pa_condensed_ops_batch) */
int pa_condensed_launch_info(pa_context *ctx, pa_degree_info di, int quad_kind, int stab_kind,
                             size_t n, pa_launch_info *out);

#ifdef __cplusplus
}
#endif
#endif
