/* blockcg_hip.h -- C ABI of libblockcg_hip.so: the MI355X (gfx950) SBCGrQ hot path.
 *
 * This is the drop-in boundary for the iteration hot path of lkeegan/blockCG.  The reference has no
 * FFI: its boundary is the header-level C++ API of inc/fields.hpp, inc/dirac_op.hpp and
 * inc/block_solvers.hpp.  Every entry point below names the reference interface it replaces
 * (file:line relative to the reference root).  The C++ classes with the reference's names
 * (blockcg_amd/include/blockcg/{fields,dirac_op,block_solvers}.hpp) are thin wrappers over these
 * calls; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *  - Plain pointers and sizes only; no C++ or torch types.  Every call returns an int status
 *    (BCG_OK = 0); the reference's assert-only error convention (inc/block_solvers.hpp:97-101)
 *    cannot cross a C ABI.  bcg_last_error() returns a message for the last failure on the context.
 *  - Scalars are complex<double> stored as interleaved (re, im) doubles.
 *  - HOST layouts at this boundary are the reference's in-memory layouts:
 *      block field  [site][rhs j][colour c]      48*m bytes per site   inc/fields.hpp:19-20,28-30
 *      m x m matrix column-major (i,j) at j*m+i                         inc/fields.hpp:22-23
 *      gauge links  [site][mu < ndim][3x3 column-major]  144 B per link inc/dirac_op.hpp:10-11
 *    Device layouts are private to the library: fields are [site][colour][rhs] so that
 *    one (site, colour) row of m complex numbers is contiguous.
 *  - Site counts and byte offsets are 64-bit: 128^4 sites fit in int, 128^4 * 768 B does not.
 *  - Block width m (the reference's template parameter N_rhs, an arbitrary int: inc/fields.hpp:19-26) is a run-time
 *    argument: any 1 <= m <= 32 (BCG_ERR_UNSUPPORTED otherwise).  m = 8, 16, 32 run the MFMA row kernels and the
 *    specialised stencil; every other width the generic kernels (one thread per output element, LDS-staged operands).
 *  - Lattice: up to 4 dimensions, lexicographic site order with x0 fastest, periodic.  ndim = 1,
 *    dims = {V} is exactly the reference's 1-D operator (inc/dirac_op.hpp:14-21); the n-D operator
 *    is  (D psi)(x) = 1/2 sum_mu eta_mu(x) [U_mu(x) psi(x+mu) - U_mu(x-mu)^dagger psi(x-mu)],
 *    eta_mu(x) = (-1)^(x_0+...+x_{mu-1})  (global coordinates).
 *  - One context = one GPU = one rank of a process grid.  With grid = {1,1,1,1} nothing
 *    communicates.  With more ranks the caller supplies two callbacks (bcg_comm) that move halo
 *    faces and sum m x m partials.  libblockcg_rccl.so (include/blockcg_rccl.h) implements them natively on RCCL
 *    (grouped ncclSend/ncclRecv, ncclAllReduce) -- what bench.py and examples/multi_gpu_solver.cpp use;
 *    blockcg_amd/comm.py is a torch.distributed implementation kept for rehearsals (gloo: ranks sharing one GPU).
 *  - All work is enqueued on the context's HIP stream; calls that return host data synchronize it.
 */
#ifndef BLOCKCG_HIP_H
#define BLOCKCG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCG_OK 0
#define BCG_ERR_INVALID 1     /* bad argument (null pointer, size mismatch, unsorted shifts ...) */
#define BCG_ERR_UNSUPPORTED 2 /* block width or lattice shape not instantiated */
#define BCG_ERR_HIP 3         /* a HIP runtime call failed; see bcg_last_error */
#define BCG_ERR_NO_DEVICE 4   /* no usable gfx950 device */
#define BCG_ERR_COMM 5        /* a communication callback failed or is missing */
#define BCG_ERR_NUMERIC 6     /* non-finite or non-positive-definite Gram matrix (CholQR breakdown) */

typedef struct bcg_context bcg_context;
typedef struct bcg_field bcg_field; /* device block field: V_local sites x 3 colours x m columns */
typedef struct bcg_gauge bcg_gauge; /* device gauge links of a dirac_op */

/* ---- communication callbacks (multi-GPU only) ------------------------------------------------
 * halo_exchange: the library has packed 2 faces per split direction into the send buffer and now
 *   needs the matching faces of the neighbour ranks in the receive buffer.  Buffers are device
 *   memory owned by the library (bcg_halo_buffers).  n_msgs messages; message k sends
 *   send_bytes[k] bytes at send_offset[k] to rank peer_send[k] and receives the same number of bytes
 *   at recv_offset[k] from rank peer_recv[k]; messages to one peer must match in posting order.
 *   The exchange must be ordered after prior work on the context's stream and complete (or be
 *   stream-ordered) before later work on it.
 * allreduce_sum: sum `count` doubles at device pointer `buf` over all ranks, in place, identically
 *   on every rank, stream-ordered as above. */
typedef struct bcg_comm {
  void* user;
  int (*halo_exchange)(void* user, int n_msgs, const int* peer_send, const int* peer_recv, const size_t* send_offset,
                       const size_t* recv_offset, const size_t* nbytes);
  int (*allreduce_sum)(void* user, void* buf, size_t count);
  /* Optional split form of halo_exchange (both NULL or both set).  begin posts the same messages, ordered after the
   * work already enqueued on the context's stream, and returns without making the stream wait; end makes the stream
   * wait for their completion.  Between the two the library enqueues the stencil over the interior tiles, which read
   * no ghost site, so the exchange overlaps that arithmetic; the boundary tiles follow end.
   * Up to TWO exchanges may be outstanding (capacity mode posts the faces of the source in two windows and the first
   * chunk's `tmp` faces behind them); halo_exchange_end ends the OLDEST one.  Their send and receive ranges are disjoint;
   * a transport may run them one after the other.  n_msgs is at most 16 (a window may consist of two x3 ranges). */
  int (*halo_exchange_begin)(void* user, int n_msgs, const int* peer_send, const int* peer_recv, const size_t* send_offset,
                             const size_t* recv_offset, const size_t* nbytes);
  int (*halo_exchange_end)(void* user);
} bcg_comm;

/* ---- context ------------------------------------------------------------------------------- */
/* device: HIP device ordinal.  stream: a hipStream_t to enqueue on, or NULL for a private stream.
 * ndim, global_dims[ndim]: the whole lattice.  grid[ndim]: ranks per direction (NULL = all 1);
 * coords[ndim]: this rank's position (NULL = all 0).  global_dims[mu] % grid[mu] must be 0. */
int bcg_context_create(bcg_context** ctx, int device, void* stream, int ndim, const int* global_dims, const int* grid,
                       const int* coords);
int bcg_context_destroy(bcg_context* ctx);
const char* bcg_last_error(const bcg_context* ctx); /* ctx may be NULL: last creation error */
int bcg_context_set_comm(bcg_context* ctx, const bcg_comm* comm);
int64_t bcg_local_volume(const bcg_context* ctx);
int bcg_local_dims(const bcg_context* ctx, int* dims4_out, int* origin4_out);
/* Pure host helper, needs no device: the message plan one halo exchange of this rank would pass to
 * bcg_comm.halo_exchange for `site_bytes` bytes per site (48*m for a field, 144 for links).  Arrays need
 * capacity 8 (2 messages per split direction).  Buffers hold, per split direction in ascending mu,
 * [minus face][plus face], each V_local/L_mu sites in lexicographic order of the other coordinates.
 * Message 2k sends the low face (x_mu = 0) to the minus neighbour and receives the plus ghost from the
 * plus neighbour; message 2k+1 sends the high face to the plus neighbour and receives the minus ghost.
 * Returns the number of messages, or a negative value for an invalid decomposition. */
int bcg_halo_plan(int ndim, const int* global_dims, const int* grid, const int* coords, size_t site_bytes, int* peer_send,
                  int* peer_recv, size_t* send_offset, size_t* recv_offset, size_t* nbytes, int64_t* ghost_sites);
/* Device halo buffers (valid after the first exchange was sized); for wrapping as communicator-visible
 * tensors. */
int bcg_halo_buffers(bcg_context* ctx, void** send, void** recv, size_t* bytes_each);
int bcg_synchronize(bcg_context* ctx);
/* The hipStream_t every call on this context enqueues on and its HIP device ordinal (for a transport that must order its
 * transfers with the library's kernels: include/blockcg_rccl.h). */
int bcg_context_stream(const bcg_context* ctx, void** stream_out, int* device_out);
/* Overlap tuning of the split halo exchange (bcg_comm.halo_exchange_begin/end).  interior_blocks: workgroups of the
 * stencil launch over the interior tiles, which runs while the exchange is in flight (default 512 = 2 per CU; a smaller
 * grid leaves compute units to the transport's kernels, at the price of a slower interior sweep; 0 keeps the current
 * value).  Results do not depend on it.  Also settable with BCG_HOP_BLOCKS_OVERLAP at context creation. */
int bcg_overlap_tuning(bcg_context* ctx, int interior_blocks);
/* Per-kernel timing with HIP events on the context's stream (off by default).  Names and
 * accumulated milliseconds / launch counts are returned as a JSON string owned by the context. */
int bcg_profiling(bcg_context* ctx, int enable);
const char* bcg_profile_json(bcg_context* ctx);
int bcg_profile_reset(bcg_context* ctx);
/* Force the generic (any-m, VALU) kernels even where an MFMA fast path exists; for parity tests. */
int bcg_force_generic(bcg_context* ctx, int enable);
/* Capacity mode.  dirac_op::op (inc/dirac_op.hpp:36-43) holds a whole field `tmp` = D P between its two stencil
 * applications.  With ring_slices = R > 0 the library keeps only R slices of `tmp` (slices of the last direction x3) and
 * runs the second application R-2 slices behind the first, so the solver's working set shrinks by (1 - R/L3) of a
 * field: what lets 128^4 sites x 16 right-hand sides x 4 shifts fit 8 x 288 GiB.  Results equal the default mode's up to
 * the summation order of the fused Gram product.  Requires a 4-D lattice whose direction 3 is not divided over ranks,
 * R >= 3 and R | L3 (else BCG_ERR_UNSUPPORTED / BCG_ERR_INVALID); applies to the widths of the specialised stencil
 * (8, 16, 32 with L0 a multiple of the tile length), other widths keep the whole `tmp`.  Halo exchanges are issued per
 * chunk of R-2 slices; when the bcg_comm offers the split form and R >= 4 they overlap the stencil work on the neighbouring
 * chunks (chunks of (R-2)/2 slices).  0 switches back. */
int bcg_capacity_mode(bcg_context* ctx, int ring_slices);
/* Device memory one SBCGrQ solve of width m with n_shifts shifts occupies on this rank in the current mode: X_s, P_s,
 * Q, T (+ the caller's B unless consume_B), tmp or its ring, links, halo buffers, scratch -- and, outside capacity mode
 * at m = 8 and 16, up to two further residual buffers and one spare field: the solver updates X_s, P_s of the
 * shifts s >= 1 (inc/block_solvers.hpp:161-181) up to four iterations at a time, which needs the residual block of
 * each deferred iteration (two at a time, as in capacity mode and at m = 32, need none: T doubles as the second buffer),
 * and X_0 (:145) with them, which needs the group's first P_0 kept in the spare field while P_0 moves on.  A single
 * system (n_shifts = 1) groups for X_0's sake alone, in threes or fours or not at all.  X_s, s >= 1, the residuals and
 * the iteration count are bit-identical to the ungrouped solver, X_0 agrees to rounding (1e-13); capacity mode (groups of
 * two) defers X_0 as well, in a form that needs no field; a solve that cannot
 * allocate the buffers runs with fewer; BCG_PAIR_SHIFTS=0 at context creation switches the grouping off, BCG_DEFER_X0=0
 * the deferred X_0 update.  Host arithmetic only. */
int bcg_sbcgrq_device_bytes(const bcg_context* ctx, int m, int n_shifts, int consume_B, size_t* bytes_out);
/* The same plan without a context or a device, for one rank of a process grid (a launcher sizing a run before it starts
 * its ranks): ring_slices = 0 for a whole `tmp`; ring_overlapped = the per-chunk exchanges overlap (split callbacks
 * present, ring >= 4); group_depth = iterations the shift updates are grouped over (1 = off, at most 4). */
int bcg_sbcgrq_plan_bytes(int ndim, const int* global_dims, const int* grid, int m, int n_shifts, int consume_B, int ring_slices,
                          int ring_overlapped, int group_depth, size_t* bytes_out);
/* ... and one HALF-VOLUME solve (bcg_field_create_half below: all work fields hold V/2 sites, links stay full-volume) */
int bcg_sbcgrq_device_bytes_half(const bcg_context* ctx, int m, int n_shifts, int consume_B, size_t* bytes_out);

/* ---- fields: block_fermion_field<N_rhs> (inc/fields.hpp:25-147) --------------------------- */
int bcg_field_create(bcg_context* ctx, int m, bcg_field** f);          /* explicit ctor :35 (contents undefined) */
int bcg_field_destroy(bcg_field* f);
int bcg_field_width(const bcg_field* f);
/* Half-volume (parity-compact) fields -- SURVEY.md section 8f-4 / Appendix D.  dirac_op::D couples nearest neighbours only
 * (inc/dirac_op.hpp:14-21), i.e. sites of opposite parity x_0+x_1+x_2+x_3 (mod 2), so dirac_op::op = mass^2 - D^2
 * (inc/dirac_op.hpp:36-43) never mixes the two parities and (op + sigma) X = B splits into two independent solves on V/2
 * sites each.  A half field holds the V/2 local sites of one parity (0 or 1) in the order of the full lattice; every
 * field primitive, dirac_apply and every solver accept half fields (all operands of a call of the SAME parity; the
 * solver's work fields are then half fields too: half the device memory of a full-volume solve, twice).
 * Even extents only (BCG_ERR_UNSUPPORTED otherwise).  Links stay full-volume.  On a lattice divided over ranks a half
 * field's ghost faces hold half the sites: the library posts the same message plan as for a full field (bcg_halo_plan) with
 * HALF the bytes per site, i.e. every offset and size halves; no capacity ring for half fields. */
int bcg_field_create_half(bcg_context* ctx, int m, int parity, bcg_field** f);
int bcg_field_parity(const bcg_field* f);   /* -1: full field; 0 / 1 */
int64_t bcg_field_sites(const bcg_field* f); /* sites held: V_local or V_local / 2 */
/* to_half != 0: half = the sites of its parity of `full`; else: those sites of `full` = half (the rest of `full` is kept) */
int bcg_field_parity_copy(bcg_field* full, bcg_field* half, int to_half);
/* The reference's fields live in host memory in the layout [site][rhs][colour] (inc/fields.hpp:19-20,28-30) and its
 * drivers read elements there (benchmark.cpp:61-63).  Both transfers convert the layout on the device and pipeline two
 * chunks (conversion kernel of one behind the bus transfer of the other).  Host memory the HIP runtime knows as pinned --
 * bcg_host_alloc below, hipHostMalloc, hipHostRegister -- is read / written by the DMA engine directly; pageable memory
 * goes through two pinned staging buffers that several host threads fill / drain. */
int bcg_field_upload(bcg_field* f, const double* host);                 /* host -> device */
int bcg_field_download(const bcg_field* f, double* host);               /* device -> host */
/* Pinned host memory for such mirrors (std::vector's allocator in the reference: Eigen::aligned_allocator,
 * inc/fields.hpp:28-30); no context needed. */
int bcg_host_alloc(size_t bytes, void** out);
int bcg_host_free(void* p);
/* operator[](int) :37-38 read access without moving the whole field: the tiles of n chosen LOCAL sites,
 * host[k] = f[sites[k]] in the host layout ([rhs][colour], 48*m bytes each).  Sites out of range: BCG_ERR_INVALID. */
int bcg_field_download_sites(const bcg_field* f, int64_t n, const int64_t* sites, double* host);
int bcg_field_copy(bcg_field* dst, const bcg_field* src);               /* copy-construct / assignment */
int bcg_field_set_zero(bcg_field* f);                                   /* setZero :57-61 */
/* i.i.d. uniform [-1,1) per real component from the counter-based generator shared with the
 * oracle (value depends on seed and GLOBAL element index only); stands in for setRandom :62-66 */
int bcg_field_fill_random(bcg_field* f, uint64_t seed);
int bcg_field_add_assign(bcg_field* y, const bcg_field* x);             /* operator+= :40-46 */
int bcg_field_sub_assign(bcg_field* y, const bcg_field* x);             /* operator-= :47-53  (K9) */
int bcg_field_add_scalar(bcg_field* y, const bcg_field* x, double a);   /* add(rhs, double) :70-77  (K3) */
int bcg_field_add_matrix(bcg_field* y, const bcg_field* x, const double* M); /* add(rhs, m x m) :70-77  (K5) */
/* rescale_add :79-90:  y = y*a + x*b  (K2) ;  y = y*M + x*b  (K6) */
int bcg_field_rescale_add_scalar(bcg_field* y, double a, const bcg_field* x, double b);
int bcg_field_rescale_add_matrix(bcg_field* y, const double* M, const bcg_field* x, double b);
/* hermitian_dot :103-122: out = a^dagger b (m x m, column-major), lower triangle mirrored so the
 * result is exactly Hermitian; summed over all ranks.  (K4) */
int bcg_field_hermitian_dot(const bcg_field* a, const bcg_field* b, double* out);
int bcg_field_real_dot(const bcg_field* a, const bcg_field* b, double* out); /* real_dot :93-99, m = 1 */
/* multiply_upper_triangular_inverse_RHS :125-136:  y <- y R^{-1}, R upper triangular  (K7) */
int bcg_field_tri_solve_rhs(bcg_field* y, const double* R);
/* thinQR :140-146:  R = chol(y^dagger y)^dagger ; y <- y R^{-1}.  BCG_ERR_NUMERIC if the Gram
 * matrix is not positive definite (the reference would silently produce NaN). */
int bcg_field_thin_qr(bcg_field* y, double* R_out);

/* ---- operator: dirac_op (inc/dirac_op.hpp:8-44) --------------------------------------------- */
int bcg_gauge_create(bcg_context* ctx, bcg_gauge** g);
int bcg_gauge_destroy(bcg_gauge* g);
int bcg_gauge_upload(bcg_gauge* g, const double* host);      /* local sites, [site][mu][3x3 col-major] */
int bcg_gauge_fill_random(bcg_gauge* g, uint64_t seed);      /* stands in for the ctor's setRandom :27-32 */
/* private D :14-21 (exposed for tests):  out = D in */
int bcg_dirac_hop(bcg_context* ctx, const bcg_gauge* g, bcg_field* out, const bcg_field* in);
/* op :36-43:  out = mass^2 in - D(D(in)).  The reference allocates a temporary per call (:39);
 * here the context owns one scratch field per width. */
/* out (parity p) = D in (parity 1 - p), half fields: the two off-diagonal blocks of dirac_op::D in the parity basis */
int bcg_dirac_hop_half(bcg_context* ctx, const bcg_gauge* g, bcg_field* out, const bcg_field* in);
int bcg_dirac_apply(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* out, const bcg_field* in);

/* ---- solver: SBCGrQ (inc/block_solvers.hpp:91-185) ------------------------------------------ */
typedef struct bcg_sbcgrq_trace {
  /* Optional per-iteration record for the first `capacity` iterations; arrays owned by caller.
   * mats: [capacity][3 + 2*n_shifts][m*m] complex column-major = alpha, rho, delta, alpha_s[], beta_s[]
   * res : [capacity][1 + n_shifts] doubles = residual, residual_shift[] (-1 = shift not visited) */
  int capacity;
  int recorded;
  double* mats;
  double* res;
} bcg_sbcgrq_trace;

/* X[n_shifts] must be fields of B's width; they are overwritten (zeroed first, :111-113).
 * sigma must be non-negative and ascending (:99-101) else BCG_ERR_INVALID.
 * eps = eps_shifts = 0 with a finite max_iterations is the fixed-work benchmark mode.
 * consume_B != 0 lets the solver use B's storage as its residual block Q (B is destroyed
 * logically; saves one field of memory at 128^4).  *iterations_out = operator applications (:184). */
int bcg_sbcgrq_solve(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* const* X, bcg_field* B, int n_shifts,
                     const double* sigma, double eps, double eps_shifts, int max_iterations, int consume_B,
                     int* iterations_out, double* residual_out, bcg_sbcgrq_trace* trace);

/* The same solver as a resumable state machine, so a caller can run (and time) an exact number of
 * iterations: begin = everything before the loop (:97-131); iterate = at most max_new_iterations
 * passes of the loop body (:132-182), stopping early when residual <= eps; end releases the work
 * fields.  X and B must outlive the state. */
typedef struct bcg_sbcgrq_state bcg_sbcgrq_state;
int bcg_sbcgrq_begin(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* const* X, bcg_field* B, int n_shifts,
                     const double* sigma, double eps, double eps_shifts, int consume_B, bcg_sbcgrq_state** state);
int bcg_sbcgrq_iterate(bcg_sbcgrq_state* state, int max_new_iterations, int* iterations_total, double* residual_out,
                       bcg_sbcgrq_trace* trace);
int bcg_sbcgrq_end(bcg_sbcgrq_state* state);

/* Sum mode, for rational functions of the operator in partial fractions (RHMC):
 *   Y = c0 B + sum_s residue[s] X_s,  X_s the solutions bcg_sbcgrq_solve would return (the solve is otherwise
 * bcg_sbcgrq_solve's, statement for statement: P_s, every coefficient, residual and the iteration count are bit-identical).
 * The X_s are never formed: each update X_s += P_s M becomes Y += P_s (residue[s] M), so the caller keeps one field
 * instead of n_shifts.  Y: a field of B's width and parity, distinct from B; Y = c0 B is written in begin, before B can
 * be consumed.  residue: n_shifts real, finite values; c0 finite (else BCG_ERR_INVALID).  A shift retired by eps_shifts
 * stops contributing, exactly as its X_s stops changing; after an error Y holds c0 B + sum_s residue[s] X_s of the last
 * completed iteration.  bcg_sbcgrq_iterate and bcg_sbcgrq_end work unchanged on the state. */
int bcg_sbcgrq_begin_sum(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* Y, bcg_field* B, int n_shifts,
                         const double* sigma, const double* residue, double c0, double eps, double eps_shifts,
                         int consume_B, bcg_sbcgrq_state** state);
int bcg_sbcgrq_solve_sum(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* Y, bcg_field* B, int n_shifts,
                         const double* sigma, const double* residue, double c0, double eps, double eps_shifts,
                         int consume_B, int max_iterations, int* iterations_out, double* residual_out,
                         bcg_sbcgrq_trace* trace);

/* ---- the callers either side of the hot path, on the same kernels ---------- */
/* True relative residuals as the reference's tests and benchmark measure them (test/solvers.cpp:104-116,
 * benchmark.cpp:93-103): res_out[s*m + i] = |(A + sigma_s) X_s - B|_i / |B|_i. */
int bcg_true_residuals(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* const* X, const bcg_field* B,
                       int n_shifts, const double* sigma, double* res_out);
/* CG  src/standard_solvers.cpp:3-32   and   SCG  src/standard_solvers.cpp:34-95   (fields of width 1).
 * SCG compares eps_shifts with the UNNORMALISED residual |r| times zeta_s, as the reference does (:90), while eps is
 * scaled by |b| (:57); the base system (shift 0) never retires and runs to eps whatever eps_shifts is. */
int bcg_cg_solve(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* x, const bcg_field* b, double eps,
                 int max_iterations, int* iterations_out);
int bcg_scg_solve(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* const* x, const bcg_field* b, int n_shifts,
                  const double* sigma, double eps, double eps_shifts, int max_iterations, int* iterations_out);
/* BCG  inc/block_solvers.hpp:10-45   and   BCGrQ  inc/block_solvers.hpp:50-86 */
int bcg_bcg_solve(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* X, const bcg_field* B, double eps,
                  int max_iterations, int* iterations_out);
int bcg_bcgrq_solve(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* X, const bcg_field* B, double eps,
                    int max_iterations, int* iterations_out);

/* Algorithmic HBM bytes of one SBCGrQ iteration on this rank's sub-lattice:
 *   V_local * [ (14 + 4*(S-1)) * 48*m + 2 * 144*ndim ] */
double bcg_sbcgrq_bytes_per_iteration(const bcg_context* ctx, int m, int n_shifts);

/* ---- fermion force of multi-shift solutions (the molecular-dynamics force of an RHMC-type integrator) ----------------
 * For a block pseudofermion B (m columns) under A = mass^2 - D^2 (bcg_dirac_apply) the action of a rational approximation is
 *   S(U) = sum_s a_s sum_j B_j^dagger (A + sigma_s)^-1 B_j,      X_s = (A + sigma_s)^-1 B   (what bcg_sbcgrq_solve returns).
 * D is anti-Hermitian for any links, so for an arbitrary complex perturbation dU of the links
 *   dS = sum_{x,mu} Re tr( dU_mu(x) G_mu(x) ),
 *   G_mu(x) = sum_s a_s eta_mu(x) sum_j [ Y_sj(x+mu) X_sj(x)^dagger - X_sj(x+mu) Y_sj(x)^dagger ],   Y_s = D X_s,
 * eta_mu as for the operator above (global coordinates), x+mu periodic; each bracket is a 3 x 3 colour outer product summed
 * over the block columns j.  (dS = sum_s a_s 2 Re X_s^dagger dD Y_s; the 1/2 of D cancels the 2.)  For an integrator that
 * moves U -> exp(eps P) U with P traceless anti-Hermitian,
 *   dS/deps = sum Re tr( P TA(U_mu(x) G_mu(x)) ),   TA(M) = (M - M^dagger)/2 - tr(M - M^dagger)/6 * 1.
 *
 * bcg_force_accumulate:  F += scale * sum_s residue[s] * G_s    (project = 0)
 *                        F += TA(U * scale * sum_s residue[s] * G_s)   (project != 0)
 * with residue[s] in the place of a_s.  F is a bcg_gauge of the same context used as a link-shaped container: layout
 * [site][mu < ndim][3x3 column-major], every local site (that of bcg_gauge_upload); its contents are added to, and its gauge
 * ghost is marked stale.  X[n_shifts]: any fields (solutions or not) of one width and one parity.  Half fields (parity p):
 * Y_s = bcg_dirac_hop_half(X_s) has parity 1 - p and every link joins one site of each parity, so F gets entries at every
 * site.  work[n_work]: fields of X's width and parity, the storage of Y_s (none may be an X_s); with n_work = 0 the library
 * allocates one for the call (BCG_ERR_HIP with F untouched if it cannot); with more, up to min(n_work, n_shifts, 8) shifts
 * share one pass over F.  Results do not depend on n_work beyond rounding.  A lattice divided over ranks exchanges the faces
 * of X_s and Y_s (blocking); arguments are checked and memory allocated before the first exchange.
 * BCG_ERR_INVALID: F == U; F, U or an X_s of another context; mixed widths or parities; n_shifts < 1; a non-finite residue
 * or scale; a work field of the wrong width or parity, listed twice, or one of the X_s. */
int bcg_force_accumulate(bcg_context* ctx, const bcg_gauge* U, bcg_field* const* X, int n_shifts, const double* residue,
                         double scale, int project, bcg_field* const* work, int n_work, bcg_gauge* F);
int bcg_gauge_download(const bcg_gauge* g, double* host); /* inverse of bcg_gauge_upload */
int bcg_gauge_set_zero(bcg_gauge* g);

/* ---- sources and sinks on the device: noise, point / wall sources, slice sums ------------------------------------------
 * What a solve starts from and what a measurement takes out of it, without a whole-field transfer.  Coordinates and slice
 * indices are GLOBAL; on a lattice divided over ranks every rank makes the same call and fills or sums the sites it holds.
 * Argument checks use global data only, so every rank returns the same status; after BCG_ERR_INVALID the field is as it was.
 *
 * Noise.  The counter generator of bcg_field_fill_random gives a complex element two uniforms a, b in [-1, 1) (its real
 * and imaginary part there); from the same two, so that a value depends on seed and the GLOBAL element index only:
 *   BCG_NOISE_GAUSSIAN  z = sqrt(-ln((1 - a) / 2)) * (cos(pi b), sin(pi b)): density exp(-|z|^2), <|z|^2> = 1, |z| <= 6.1
 *   BCG_NOISE_Z2        z = (a < 0 ? -1 : +1, 0)
 *   BCG_NOISE_Z4        z = ((a < 0 ? -1 : +1), (b < 0 ? -1 : +1)) / sqrt(2)
 * Half fields get the values the full field has on their sites.  Unknown kind: BCG_ERR_INVALID. */
#define BCG_NOISE_GAUSSIAN 0
#define BCG_NOISE_Z2 1
#define BCG_NOISE_Z4 2
int bcg_field_fill_noise(bcg_field* f, int kind, uint64_t seed);
/* f = 0, then column j has a 1 at site coords[4*j .. 4*j+3] (entries beyond ndim must be 0), colour colour[j].
 * BCG_ERR_INVALID: a coordinate outside the global lattice, a colour outside 0..2, on a half field a site of the other parity. */
int bcg_field_set_point_sources(bcg_field* f, const int* coords, const int* colour);
/* f = 0, then column j has a 1 in colour colour[j] on every site with x_dir = slice[j] whose parity x_0+x_1+x_2+x_3 (mod 2)
 * is site_parity (-1: every site of the slice).  A half field accepts -1 or its own parity.  One pass over f.
 * BCG_ERR_INVALID as above, or dir outside 0 .. ndim-1. */
int bcg_field_set_wall_sources(bcg_field* f, int dir, const int* slice, const int* colour, int site_parity);
/* out[t*m + j] = sum_{x: x_dir = t} sum_c conj(a[x,c,j]) b[x,c,j], t over the GLOBAL extent of direction dir, interleaved
 * (re, im): the diagonal of bcg_field_hermitian_dot resolved by slice.  Summed over all ranks (bcg_comm.allreduce_sum) and
 * identical on every rank; the same bits on every call (fixed blocks per slice, block sums added in a fixed order, no
 * atomics).  a == b reads the field once.  Half fields: both operands of one parity, the sites held contribute.
 * BCG_ERR_INVALID: mixed widths, parities or contexts, dir outside 0 .. ndim-1; BCG_ERR_UNSUPPORTED: more than 2^20 / m
 * slices.  Synchronizes the stream. */
int bcg_field_slice_dot(const bcg_field* a, const bcg_field* b, int dir, double* out);
/* Per-slice Gram matrices with momentum projection: all column pairs of bcg_field_hermitian_dot resolved by slice,
 *   out[((p*L_dir + t)*m + j)*m + i] = sum_{x: x_dir = t} w_p(x) sum_c conj(a[x,c,i]) b[x,c,j],
 *   w_p(x) = exp(-2 pi i sum_{mu != dir} n_{p,mu} x_mu / L_mu),      n_{p,mu} = momenta[4*p + mu],
 * interleaved (re, im); t, x_mu and L_mu are GLOBAL coordinates and extents, each (p, t) block an m x m matrix, column-major.
 * n_mom = 0 (momenta may be NULL): the single momentum 0, no phase arithmetic at all.  Momenta are any integers, reduced
 * mod L_mu exactly; the phase of a site is the product over ascending mu of entries exp(-2 pi i ((n_mu x_mu) mod L_mu) / L_mu)
 * of per-direction tables computed on the host in double precision, so no value depends on the process grid.
 * Summed over all ranks (one bcg_comm.allreduce_sum per chunk of momenta) and identical on every rank; the same bits on
 * every call (a launch plan fixed by shape, width, parity, dir and n_mom; block sums added in a fixed order; no atomics).
 * Full and half fields (both operands of one parity; the sites held contribute), every width 1..32; a == b reads the field
 * once; a and b are not written.  Uses the context's existing scratch only.
 * BCG_ERR_INVALID: mixed widths, parities or contexts, dir outside 0 .. ndim-1, n_mom < 0, n_mom > 0 with momenta == NULL,
 * out == NULL, a non-zero momentum component along dir or along a direction >= ndim; BCG_ERR_UNSUPPORTED: the L_dir m^2
 * entries of one momentum do not fit the scratch (2^20 entries); BCG_ERR_COMM: a divided lattice without a bcg_comm.  A
 * failed call leaves out untouched.  Synchronizes the stream. */
int bcg_field_slice_gram(const bcg_field* a, const bcg_field* b, int dir, int n_mom, const int* momenta, double* out);

/* ---- covariant shifts, Laplacian and smearing (extensions) ---------------------------------------
 * The nearest-neighbour sum with free coefficients,
 *   out(x) = c0 in(x) + sum_mu s_mu(x) [ fwd[mu] U_mu(x) in(x+mu) + bwd[mu] U_mu(x-mu)^dagger in(x-mu) ],
 * c0 = (re, im), fwd and bwd = ndim x (re, im) (NULL: all 0); s_mu(x) = eta_mu(x) = (-1)^(x_0+...+x_{mu-1}) in GLOBAL
 * coordinates when eta != 0, and 1 otherwise.  Sites are periodic and links general complex 3 x 3, as everywhere here.
 *  - Zero coefficients: a term whose coefficient is exactly 0 (re and im) is not evaluated.  A direction with
 *    fwd[mu] == bwd[mu] == 0 reads neither its links nor its neighbour rows, so non-finite data in such links never reaches
 *    out; c0 == 0 does not read in(x).
 *  - A direction of extent 1 has the site itself as both neighbours (as in bcg_dirac_hop).
 *  - With c0 = 0, fwd = 1/2, bwd = -1/2, eta = 1 the call is bcg_dirac_hop to rounding (not bit for bit).
 *  - g: an operator's links or any link-shaped bcg_gauge of the context (e.g. links smeared on the device by bcg_gauge_stout_smear);
 *    a stale gauge ghost is refreshed first, as by bcg_dirac_hop.
 *  - Full fields: out and in distinct full fields of one width and context.  Half fields: in of parity p, out of parity
 *    1 - p, c0 exactly 0; even extents and half ghost faces as for bcg_dirac_hop_half.
 *  - Divided lattices: one blocking exchange of in's faces per call; every rank makes the same call; the argument checks
 *    use global data only, so every rank returns the same status.
 *  - BCG_ERR_INVALID: a NULL out, in, g or c0; out == in; mixed widths or contexts; wrong parities; a non-zero c0 with half
 *    fields; a non-finite coefficient.  BCG_ERR_COMM: a divided lattice without a bcg_comm.  The arguments are checked
 *    before the first launch or exchange: a call that fails them leaves out as it was (a BCG_ERR_HIP or BCG_ERR_COMM from
 *    the exchange or the launch itself leaves out undefined).
 *  - Profile key "shift_sum": 2 * 48 m bytes per site of out plus 144 bytes per site and direction with a non-zero
 *    coefficient, and the flops of the terms evaluated ("shift_form_tile" / "shift_form_generic" count the kernel form). */
int bcg_dirac_shift_sum(bcg_context* ctx, const bcg_gauge* g, bcg_field* out, const bcg_field* in,
                        const double* c0 /* (re, im) */, const double* fwd /* ndim x (re, im), NULL = all 0 */,
                        const double* bwd /* likewise */, int eta);
/* f <- (1 + kappa * Lap_dir)^n_iter f,  Lap_dir psi = sum_{mu != dir} [U psi(x+mu) + U^dagger psi(x-mu) - 2 psi];
 * dir = -1: every direction.  Exactly n_iter calls of bcg_dirac_shift_sum with c0 = 1 - 2 kappa (number of smeared
 * directions), fwd = bwd = kappa on the smeared directions, 0 on dir, eta = 0, alternating between f and work; the result
 * ends in f (after an odd number of steps by a device copy) and is bit-identical to the same calls made by hand.
 * work: a field of f's width (NULL: allocated for the call); contents undefined afterwards.  n_iter = 0 leaves f untouched.
 * Full fields only: a half field returns BCG_ERR_UNSUPPORTED, because one link flips the parity.  "smear" is no profile key
 * of its own: the steps are timed as "shift_sum".
 * BCG_ERR_INVALID: a NULL g or f; mixed contexts; dir outside -1 .. ndim-1; n_iter < 0; a non-finite kappa; work == f; a
 * work of another width or parity.  BCG_ERR_COMM: a divided lattice without a bcg_comm.  These are checked before the first
 * launch or exchange, and a call that fails them leaves f as it was.  A BCG_ERR_HIP or BCG_ERR_COMM from a launch or an
 * exchange part-way through the steps leaves the contents of f (and of work) undefined. */
int bcg_covariant_smear(bcg_context* ctx, const bcg_gauge* g, bcg_field* f, bcg_field* work, int dir, double kappa,
                        int n_iter);

/* ---- gauge links: stout smearing and plaquettes (extensions) ---------------------------------------
 * Sites are periodic and links general complex 3 x 3, layout [site][mu < ndim][3x3 column-major], as everywhere here.
 * rho is an ndim x ndim table of real weights, row-major, rho[mu*ndim + nu]; its diagonal is ignored and rho[mu][nu] need
 * not equal rho[nu][mu].  A direction of GLOBAL extent 1 takes no part, neither as mu nor as nu (unlike
 * bcg_dirac_shift_sum: a staple through a direction of extent 1 is not a staple).  One step U -> U' is
 *   C_mu(x)  = sum_{nu != mu} rho[mu][nu] * [ U_nu(x) U_mu(x+nu) U_nu(x+mu)^dagger
 *                                           + U_nu(x-nu)^dagger U_mu(x-nu) U_nu(x-nu+mu) ]
 *   Omega    = C_mu(x) U_mu(x)^dagger
 *   Q        = (i/2) (Omega^dagger - Omega) - (i/6) tr(Omega^dagger - Omega) * 1      (Hermitian, traceless for ANY U)
 *   U'_mu(x) = exp(iQ) U_mu(x)
 *  - A term whose rho[mu][nu] is exactly 0 is not evaluated and its links are not read (the zero-coefficient convention of
 *    bcg_dirac_shift_sum), so non-finite data in links that no term names never reaches out.
 *  - A direction mu whose whole row of rho is 0 (after the rules above), or whose extent is 1, is copied bit for bit.
 *  - exp(iQ) = f0 + f1 Q + f2 Q^2 in the Cayley-Hamilton form of Morningstar and Peardon, exact to rounding for every
 *    Hermitian traceless Q, Q = 0 and Q with two equal eigenvalues included (DESIGN.md section 8m lists the guards).
 *
 * bcg_gauge_stout_smear: out = S^n_steps(in).  in is not written and may be an operator's links.  The steps alternate between
 * out and work so that the last one writes out, with no final copy; n_steps = 0 (or a table without a single live term) is a
 * device copy of in to out.  work: a container of the context, contents undefined afterwards; NULL: allocated for the call
 * when n_steps >= 2.  The result does not depend on whether work was passed: the same bits.  out's gauge ghost is marked
 * stale.  Divided lattices: two blocking exchanges per step (the faces of all ndim links, then the backward staples
 * U_nu^dagger U_mu U_nu(+mu) of the high faces, so no corner message is needed); every rank makes the same call, the checks
 * use global data only, and memory is allocated (and agreed on) before the first launch or exchange.
 *  - BCG_ERR_INVALID: a NULL ctx, out, in or rho; out == in, work == out or work == in; a container of another context;
 *    n_steps < 0; a non-finite entry of rho off the diagonal.  BCG_ERR_COMM: a divided lattice without a bcg_comm.
 *    BCG_ERR_UNSUPPORTED: V_local * ndim >= 2^31.  A call that fails these checks leaves out as it was.
 *  - Profile key "stout_smear", one entry per step: 2 * 144 ndim bytes per site (every link read once and written once);
 *    flops 936 per evaluated (mu, nu) term and site (four 3 x 3 products, two scaled sums) plus 798 per smeared link (Omega,
 *    Q^2, the final product, the coefficients and the polynomial).
 *
 * bcg_gauge_plaquette: for mu < nu, both of extent > 1,
 *   out[mu*ndim + nu] = out[nu*ndim + mu] = (1 / (3 V_global)) sum_x Re tr[ U_mu(x) U_nu(x+mu) U_mu(x+nu)^dagger U_nu(x)^dagger ]
 * and every other entry of out is 0.  Summed over all ranks with one bcg_comm.allreduce_sum and identical on every rank; the
 * same bits on every call (fixed blocks, block sums added in a fixed order, no atomics, as bcg_field_slice_dot).  Refreshes
 * nothing and writes nothing to g (a divided lattice exchanges the link faces into a buffer of the call).  Synchronizes the
 * stream.  BCG_ERR_INVALID: a NULL argument or links of another context; BCG_ERR_COMM: a divided lattice without a bcg_comm.
 *  - Profile key "plaquette": 144 ndim bytes per site, 468 flops per plane and site. */
int bcg_gauge_stout_smear(bcg_context* ctx, bcg_gauge* out, const bcg_gauge* in, const double* rho /* ndim*ndim */,
                          int n_steps, bcg_gauge* work /* NULL: allocated for the call when n_steps >= 2 */);
int bcg_gauge_plaquette(bcg_context* ctx, const bcg_gauge* g, double* out /* ndim*ndim */);

/* ---- products with a basis of another width (extensions) ----------------------------------------
 * V is a list of nv >= 1 fields of one context, of any widths 1 .. 32, with the parity and site count of b / y.  K is the
 * sum of the widths; basis column i is column i - offset_k of the field it falls in.  K x m matrices cross the ABI
 * column-major, interleaved (re, im), as everywhere else.  The host walks V in groups of consecutive fields, one launch per
 * group, so that b is read once (y read and written once) per group and not per field.  m in {16, 32} and widths in
 * {16, 32} take the MFMA form (up to 64 basis columns per launch at m = 16; 32 for the dot and 48 for the update at m = 32),
 * every other combination and bcg_force_generic the generic form (up to 32 columns per launch); one call may use both.  No
 * atomics: the same bits on every call.
 *  - Profile keys "basis_dot" (48 (K_g + m) bytes per site and group) and "basis_axpy" (48 (K_g + 2 m), or 48 (K_g + m)
 *    for a first group with beta == 0), 8 K_g m flops per row; "basis_form_mfma" / "basis_form_generic" count the launches
 *    of either form.
 *  - The K x m result and the uploaded coefficients live in a buffer of the context's own (device and pinned host, 16 K m
 *    bytes each), allocated on first use, grown when a larger K m arrives, freed by bcg_context_destroy.
 *
 * bcg_basis_dot: out[j*K + i] = sum_{x,c} conj(V_i(x,c)) b_j(x,c); every entry is computed, nothing is mirrored.  Block
 * partials are summed in ascending block order, then over ranks with ONE bcg_comm.allreduce_sum of the whole matrix:
 * identical on every rank.  b may be one of the V_k.  Synchronizes the stream.
 * bcg_basis_axpy: y <- beta y + sum_i V_i C(i, .), C of size K x m.  beta exactly 0 does not read y (a NaN there does not
 * survive).  y must not be one of the V_k.
 * bcg_field_copy_columns: columns src_first .. src_first + n - 1 of src go to columns dst_first .. of dst; the other
 * columns of dst keep their bits.  The widths may differ; full or half fields of one parity; dst != src.
 * BCG_ERR_INVALID: a NULL pointer, nv < 1, mixed contexts, parities or site counts, y among the V_k, dst == src, n < 1 or a
 * column range outside a field, a non-finite beta.  BCG_ERR_COMM (bcg_basis_dot): a divided lattice without a bcg_comm.
 * The arguments are checked before the first launch: a call that fails them leaves out / y / dst exactly as they were.
 *
 * bcg_basis_slice_dot: bcg_basis_dot resolved by slice and momentum,
 *   out[((p*L_dir + t)*m + j)*K + i] = sum_{x: x_dir = t} w_p(x) sum_c conj(V_i(x,c)) b_j(x,c),
 * V, K and the column numbering as above; w_p, momenta[4*p + mu], n_mom = 0 (the single momentum 0, no phase arithmetic),
 * the GLOBAL t and coordinates and the host-computed phase tables exactly as in bcg_field_slice_gram.  Each (p, t) block
 * is a K x m matrix, column-major, interleaved (re, im); every entry is computed.  Full and half fields (all operands of one
 * parity), every width 1 .. 32 on either side, divided lattices; b may be one of the V_k; nothing is written but out.
 * A call is a set of launches, each (a group of K_g basis columns) x (pc momenta), reading 48 (K_g + m) bytes per site.
 * m in {16, 32} against widths in {16, 32} take the MFMA form, whose groups are runs of 16-column blocks (a 32-wide field
 * may be split) with (K_g / 16) * pc * (m / 16) <= 4: momenta first (pc the largest of 1, 2, 4 at m = 16, of 1, 2 at m = 32,
 * that is <= max(n_mom, 1)), then the largest group left.  Every other combination and bcg_force_generic take the generic
 * form (pc 1 or 2, up to 32 columns).  Without momenta V = 2 x 32 columns at m = 16 is one launch with the bytes of
 * bcg_basis_dot.  No atomics: the launch plan is fixed by shape, widths, m, parity, dir and n_mom and the block partials of
 * a (p, t) are added in ascending order, so the same bits on every call and on every rank.  The whole P x L_dir x K x m
 * result is assembled on the device in the buffer of bcg_basis_dot, summed over ranks with ONE bcg_comm.allreduce_sum and
 * copied out once.  Synchronizes the stream.
 *  - Profile keys "basis_slice_dot" (48 (K_g + m) bytes per site and launch, 8 K_g m pc flops per row), "basis_slice_fold",
 *    "basis_slice_form_mfma" / "basis_slice_form_generic" (launch counts).
 *  - BCG_ERR_INVALID: everything bcg_basis_dot and bcg_field_slice_gram reject -- a NULL pointer, nv < 1, mixed contexts,
 *    parities or site counts, dir outside 0 .. ndim-1, n_mom < 0, n_mom > 0 with momenta == NULL, a non-zero momentum
 *    component along dir or along a direction >= ndim.  BCG_ERR_COMM: a divided lattice without a bcg_comm.
 *    BCG_ERR_UNSUPPORTED: more than 2^26 entries in all (split the momenta), or one block per slice of the smallest launch
 *    (one block of 16 columns or one generic field, one momentum) does not fit the context's scratch.  All are returned
 *    before the first launch and leave out untouched.
 *
 * bcg_basis_slice_axpy: the adjoint of bcg_basis_slice_dot, a basis put onto slices,
 *   y_j(x,c) <- beta y_j(x,c) + w(x) sum_i V_i(x,c) C_s(i, j)    on the sites with GLOBAL x_dir = slices[s],
 *   y_j(x,c) <- beta y_j(x,c)                                     on every other site,
 * V, K and the column numbering as above; y of any width m in 1 .. 32 and none of the V_k; full and half fields (all operands
 * of one parity), divided lattices.  slices: n_slices distinct global slice indices in 0 .. L_dir-1 in any order; n_slices = 0
 * with slices = NULL: all L_dir slices in ascending order.  C[(s*m + j)*K + i], interleaved (re, im): one K x m column-major
 * matrix per listed slice -- the layout of one momentum block of bcg_basis_slice_dot's out, so that with n_slices = 0 the
 * output of that call is valid input to this one.  momentum: NULL (w = 1, no phase arithmetic) or four integers, the
 * components along dir and beyond ndim 0; w(x) = conj(w_p(x)) = exp(+2 pi i sum_mu n_mu x_mu / L_mu) of the GLOBAL
 * coordinates, from the tables of bcg_field_slice_gram conjugated entry by entry on the host and multiplied in ascending
 * direction: no value depends on the process grid, and the call is the exact adjoint of bcg_basis_slice_dot at the same
 * momentum.  A distillation source is the call with one slice, beta = 0 and C a column selection; with C = tau(t) of
 * bcg_basis_slice_dot it is the per-slice projector V(t) V(t)^dagger b.
 * beta exactly 0 reads no site of y (a NaN there does not survive; the slices not listed come out as exact zeros); beta
 * exactly 1 neither reads nor writes the slices not listed; any other finite beta scales them.  Purely local: no bcg_comm
 * call; a rank that holds none of the listed slices launches nothing at beta = 1.  Does not synchronize the stream (unless
 * the coefficient buffer has to grow), as bcg_basis_axpy.
 * The groups and the two forms are those of bcg_basis_axpy; a launch walks the listed local slices only, reading
 * 48 (K_g + m) bytes per listed site; the first group's launch carries beta, the later ones run at beta = 1.  The slices not
 * listed are one streaming launch of their own at beta != 1.  Nothing is reduced: the same bits on every call.
 *  - Profile keys "basis_slice_axpy" (48 (K_g + 2 m) bytes per listed site and launch, 48 (K_g + m) for a first group with
 *    beta == 0; 8 K_g m flops per row), "basis_slice_axpy_form_mfma" / "basis_slice_axpy_form_generic" (launch counts),
 *    "basis_slice_scale" (the slices not listed).
 *  - BCG_ERR_INVALID: everything bcg_basis_axpy rejects -- a NULL pointer, nv < 1, mixed contexts, parities or site counts,
 *    y among the V_k, a non-finite beta -- and dir outside 0 .. ndim-1, n_slices < 0, n_slices > 0 with slices == NULL, a
 *    slice outside 0 .. L_dir-1 or listed twice, a non-zero momentum component along dir or along a direction >= ndim.
 *    BCG_ERR_UNSUPPORTED: more than 2^26 entries of C, or a slice of 2^30 rows or more.  All are returned before the first
 *    launch and leave y exactly as it was.
 *
 * bcg_basis_slice_triple: the baryon elementals of three lists of fields, slice by slice,
 *   out[(((p*S + s)*Kc + k)*Kb + j)*Ka + i] = sum_{x: x_dir = slices[s]} w_p(x) sum_{abc} eps_abc A_i(x,a) B_j(x,b) C_k(x,c),
 * interleaved (re, im): the colour determinant of three columns summed over a slice.  A, B, C: lists as V above (widths
 * 1 .. 32, columns numbered through the list), Ka, Kb, Kc <= 64 columns each, all fields of one context, parity and site
 * count; the lists may share fields or be the same list.  dir, n_slices, slices as in bcg_basis_slice_axpy (distinct GLOBAL
 * indices in any order; n_slices = 0: all L_dir slices ascending, S = L_dir); only the listed slices are walked.  n_mom,
 * momenta, w_p and the host phase tables exactly as in bcg_basis_slice_dot.  Nothing is written but out.
 * A launch is one momentum; a block owns one tile of the result (16^3 entries in the MFMA form: every width of the three
 * lists in {16, 32} and bcg_force_generic not set; 8^3 in the generic form) on a chunk of one slice, forms the cross product
 * A_i x B_j of a site in registers and contracts it with w C_k.  Identical lists (na == nb == nc and the same handles element
 * by element): only tiles in ascending order are launched, only the entries i < j < k are kept and each is written with its
 * five signed images, so out is antisymmetric bit for bit and exactly 0 where two indices coincide.  No atomics: the plan is
 * fixed by shape, widths, parity, dir, the listed slices and n_mom, and the block partials of a (p, s, tile) are added in
 * ascending order: the same bits on every call.  The result is assembled on the device, summed over ranks with ONE
 * bcg_comm.allreduce_sum and copied out once, identical on every rank.  Synchronizes the stream.
 *  - Profile keys "basis_slice_triple" (48 * 3 * edge bytes and 24 * edge^3 flops per listed site, tile and launch),
 *    "basis_slice_triple_fold", "basis_slice_triple_form_mfma" / "basis_slice_triple_form_generic" (launch counts).
 *  - BCG_ERR_INVALID: everything bcg_basis_dot rejects about a list (NULL, n < 1, mixed contexts, parities or site counts),
 *    everything bcg_basis_slice_axpy rejects about dir and slices, everything bcg_basis_slice_dot rejects about momenta, a
 *    NULL out.  BCG_ERR_COMM: a divided lattice without a bcg_comm.  BCG_ERR_UNSUPPORTED: a list of more than 64 columns,
 *    more than 2^26 entries in all (split the slices or the momenta), a slice of 2^30 rows or more, or so many listed slices
 *    that one block per (slice, tile) exceeds 2^24 entries of block partials.  All are returned before the first launch and
 *    leave out untouched. */
int bcg_basis_dot(const bcg_field* const* V, int nv, const bcg_field* b, double* out);
int bcg_basis_slice_dot(const bcg_field* const* V, int nv, const bcg_field* b, int dir, int n_mom, const int* momenta, double* out);
int bcg_basis_axpy(bcg_field* y, const bcg_field* const* V, int nv, const double* C, double beta);
int bcg_basis_slice_axpy(bcg_field* y, const bcg_field* const* V, int nv, int dir, int n_slices, const int* slices, const double* C,
                         const int* momentum, double beta);
int bcg_basis_slice_triple(const bcg_field* const* A, int na, const bcg_field* const* B, int nb, const bcg_field* const* C, int nc, int dir,
                           int n_slices, const int* slices, int n_mom, const int* momenta, double* out);
int bcg_field_copy_columns(bcg_field* dst, int dst_first, const bcg_field* src, int src_first, int n);

/* ---- low modes: the in-place basis rotation and the eigensolver built on it (extensions) ----------
 * bcg_basis_rotate: V <- V Q in place.  V as in bcg_basis_dot (one context, parity and site count, widths 1 .. 32, no field
 * twice), K the sum of the widths, at most BCG_BASIS_ROTATE_MAX_COLUMNS; Q is K x K, column-major, interleaved (re, im),
 * and need not be unitary.  Column j of the result is sum_i V_i Q(i, j).  One launch takes all K columns: a 16-row tile of
 * every column is read, the outputs formed from that copy and stored over their inputs -- no workspace, no second copy of
 * the basis.  Every width in {16, 32} takes the MFMA form, every other width list and bcg_force_generic the generic one.
 * Purely local (no communication call), no atomics: the same bits on every call.  A permutation matrix moves columns bit
 * for bit.  Profile keys "basis_rotate" (96 K bytes per site, 8 K^2 flops per row), "basis_rotate_mfma" /
 * "basis_rotate_generic" (launch counts).  The uploaded Q lives in a buffer of the context's own (64 x 64 entries, device
 * and pinned host), allocated on first use, freed by bcg_context_destroy.
 * BCG_ERR_INVALID: a NULL pointer, nv < 1, a field listed twice, mixed contexts, parities or site counts, a non-finite Q.
 * BCG_ERR_UNSUPPORTED: K > 64.  Either is returned before the first launch and leaves V exactly as it was.
 *
 * bcg_spectral_bound: an upper bound on the largest eigenvalue of dirac_op::op (full fields: parity -1; the block of one
 * parity: 0 / 1) from `steps` (2 .. 64) Lanczos steps on one column started from bcg_field_fill_noise(GAUSSIAN, seed):
 * theta_max(T_k) + beta_k, the safeguarded bound of Zhou and Saad.  Allocates and frees three fields of width 1.
 *
 * bcg_lowest_modes: Chebyshev-filtered subspace iteration for the lowest eigenpairs of dirac_op::op.
 *   V           in: the start block (the caller fills it, e.g. with noise); out: orthonormal Ritz vectors, Ritz values
 *               ascending over the K columns.  K <= 64; wider bases are built 64 at a time with `locked`.
 *   locked      NULL / 0, or orthonormal, already converged vectors of any total width: V is kept orthogonal to them.
 *   n_want      the first n_want columns decide convergence: max_i resid_i <= tol * upper_bound.  The filter damps
 *               everything above the largest Ritz value of the block it carries, so the top columns of that block converge
 *               slowly or not at all: the wanted columns need columns beyond them.  Half as many spare columns as wanted
 *               ones is a good start.  With n_want == K the caller brings none, and the call carries a guard block of its
 *               own: one more field of min(16, 64 - K) columns of noise (a fixed seed, a function of the global site),
 *               allocated for the call, filtered, orthonormalised and rotated with V and dropped at the end; V gets the
 *               lowest K of the K + guard Ritz vectors.  K == 64 leaves no room for one.
 *   degree      of the Chebyshev polynomial per outer iteration (>= 2); upper_bound: of the spectrum (bcg_spectral_bound).
 *   evals_out, resid_out   K each: Ritz values and ||A v_i - theta_i v_i|| of the vectors left in V.
 *   iterations_out         filter applications made; applications_out: calls of the block operator, one per field and
 *                          application: nf (2 (iterations + 1) + degree iterations), nf = nv, or nv + 1 with the guard
 *                          block.  Either may be NULL.
 * An outer iteration: project out the locked vectors, G = V^dagger V, Cholesky, V <- V R^-1; the same again with
 * H = V^dagger A V beside it and V <- V R^-1 Z from the reduced eigenproblem (two rotations per iteration in all); residuals
 * from A v - theta v itself; then, unless converged, the filter that damps [theta_K, upper_bound].  Reaching
 * max_iterations is not an error: BCG_OK, and resid_out tells.  The call allocates and frees three work fields of the
 * widest width.  Every branch is taken on all-reduced data: all ranks of a divided lattice return the same status.
 * BCG_ERR_INVALID: a NULL pointer, nv < 1, a field twice, a locked field that is also in V, mixed contexts, parities or site
 * counts, n_want outside 1 .. K, degree < 2, max_iterations < 0, a tol or upper_bound that is not finite and positive.
 * BCG_ERR_UNSUPPORTED: K > 64.  Both before anything is launched.  BCG_ERR_NUMERIC: V^dagger V not positive definite (the
 * block lost rank), a Ritz value at or above upper_bound, or Ritz values that do not spread; V then holds the
 * block as the failed step found it (same span, not orthonormal), evals_out / resid_out the last completed Ritz step. */
#define BCG_BASIS_ROTATE_MAX_COLUMNS 64
int bcg_basis_rotate(bcg_field* const* V, int nv, const double* Q);
int bcg_spectral_bound(bcg_context* ctx, const bcg_gauge* g, double mass, int parity, int steps, uint64_t seed,
                       double* bound_out);
int bcg_lowest_modes(bcg_context* ctx, const bcg_gauge* g, double mass, bcg_field* const* V, int nv,
                     const bcg_field* const* locked, int nlocked, int n_want, int degree, double upper_bound, double tol,
                     int max_iterations, double* evals_out, double* resid_out, int* iterations_out,
                     int64_t* applications_out);

/* ---- the distillation basis: per-slice rotation and Laplacian modes (extensions) -----------------
 * bcg_basis_slice_rotate: V(x) <- V(x) Q_s in place on the sites with GLOBAL x_dir = slices[s]: bcg_basis_rotate with one
 * matrix per slice.  V as in bcg_basis_rotate (one context, parity and site count, widths 1 .. 32, no field twice, K <=
 * BCG_BASIS_ROTATE_MAX_COLUMNS); dir, n_slices and slices as in bcg_basis_slice_axpy (distinct global indices in any order;
 * n_slices = 0 with slices = NULL: all L_dir slices ascending).  Q[(s*K + j)*K + i], interleaved (re, im): one column-major
 * K x K matrix per listed slice; the matrices need not be unitary.  Sites of slices that are not listed are neither read
 * nor written; a half field along direction 0 skips the other parity's sites.  Full and half fields, divided lattices.
 * Purely local: no bcg_comm call, and a rank that holds none of the listed slices launches nothing.  One launch takes all K
 * columns of the listed local slices on the walk of bcg_basis_slice_axpy; every width in {16, 32} takes the MFMA form, every
 * other width list and bcg_force_generic the generic one.  No atomics and nothing reduced: the same bits on every call.
 * Where Q_s is a permutation matrix or the identity, the columns of that slice move bit for bit.  Does not synchronize the
 * stream (unless the matrix buffer has to grow).  The matrices of the local listed slices and the slice list go through the
 * buffer of bcg_basis_rotate, grown when a call needs more and freed by bcg_context_destroy.
 *  - Profile keys "basis_slice_rotate" (96 K bytes per listed site, 8 K^2 flops per row), "basis_slice_rotate_mfma" /
 *    "basis_slice_rotate_generic" (launch counts).
 *  - BCG_ERR_INVALID: everything bcg_basis_rotate rejects (a NULL pointer, nv < 1, a field twice, mixed contexts, parities or
 *    site counts, a non-finite Q), dir outside 0 .. ndim-1, n_slices < 0, n_slices > 0 with slices == NULL, a slice outside
 *    0 .. L_dir-1 or listed twice.  BCG_ERR_UNSUPPORTED: K > 64, or a slice of 2^30 rows or more.  All are returned before
 *    the first launch and leave V exactly as it was.
 *
 * bcg_laplacian_modes: the lowest eigenpairs of A = -Lap_dir on every slice of direction dir at once,
 *   A psi(x) = 2 (ndim-1) psi(x) - sum_{mu != dir} [U_mu(x) psi(x+mu) + U_mu(x-mu)^dagger psi(x-mu)],
 * bcg_dirac_shift_sum with a zero coefficient along dir (the links of direction dir are not read).  A is Hermitian for any
 * links and block-diagonal over the slices of dir, so every slice has its own eigenproblem; the call is bcg_lowest_modes
 * slice by slice: per-slice Gram and projected matrices (bcg_basis_slice_dot), per-slice Cholesky and Ritz rotations
 * (two bcg_basis_slice_rotate calls over all slices per outer iteration), per-slice residuals (bcg_field_slice_dot).
 *   V, locked, n_want, degree, tol, max_iterations, the guard block (n_want == K: min(16, 64 - K) columns of fixed-seed
 *               noise by global site) and the counting: as in bcg_lowest_modes.  locked: orthonormal PER SLICE, any total width.
 *   upper_bound of the spectrum of A, from the caller: 4 (ndim-1) bounds it for unitary links; general (e.g. smeared,
 *               unprojected) links need a bound of the caller's own.
 *   evals_out, resid_out   L_dir x K each ([t*K + i], t the GLOBAL slice): Ritz values ascending per slice, and
 *               ||A v_i - theta_i(t) v_i|| over the sites of slice t.
 *   iterations_out, applications_out   filter applications; bcg_dirac_shift_sum calls, nf (2 (iterations + 1) + degree
 *               iterations), nf = nv, or nv + 1 with the guard block.  Either may be NULL.
 * Converged when the maximum over all slices and the first n_want columns of resid is <= tol * upper_bound.  The filter is
 * ONE Chebyshev polynomial for all slices, damping [max_t theta_last(t), upper_bound] and scaled at min_t theta_1(t), so its
 * coefficients are global and a step is one bcg_dirac_shift_sum plus one axpby.  Reaching max_iterations is no error.
 * Allocates and frees three work fields of the widest width.  Every branch is taken on all-reduced data: every rank of a
 * divided lattice, divided along dir or not, returns the same status.
 * BCG_ERR_INVALID: everything bcg_lowest_modes rejects, and dir outside 0 .. ndim-1.  BCG_ERR_UNSUPPORTED: K > 64; half
 * fields (one hop flips the parity, as in bcg_covariant_smear).  Both before anything is launched.  BCG_ERR_NUMERIC: on any
 * slice, V(t)^dagger V(t) not positive definite, a Ritz value at or above upper_bound, or Ritz values that do not spread;
 * V, evals_out and resid_out then as bcg_lowest_modes leaves them. */
int bcg_basis_slice_rotate(bcg_field* const* V, int nv, int dir, int n_slices, const int* slices, const double* Q);
int bcg_laplacian_modes(bcg_context* ctx, const bcg_gauge* g, int dir, bcg_field* const* V, int nv,
                        const bcg_field* const* locked, int nlocked, int n_want, int degree, double upper_bound,
                        double tol, int max_iterations, double* evals_out /* L_dir x K */,
                        double* resid_out /* L_dir x K */, int* iterations_out, int64_t* applications_out);

#ifdef __cplusplus
}
#endif
#endif /* BLOCKCG_HIP_H */
