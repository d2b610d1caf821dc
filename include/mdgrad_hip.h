/*
 * mdgrad_hip.h -- C ABI of libmdgrad_hip.so: the MI355X (gfx950) hot path of the
 * differentiable-MD inner loop (force evaluation + integrator + adjoint + RDF + SchNet
 * message passing), hand-written HIP.  This header is the drop-in boundary: plain
 * pointers and sizes, no torch types.  All pointers are DEVICE pointers (HIP, fp32 /
 * int32 unless stated) except where marked `host`; `stream` is a hipStream_t passed as
 * void*.  Every entry point enqueues on `stream` and returns without synchronising;
 * the return value is 0 on success or a negative MDG_E* code (mdg_last_error() gives
 * the message).  Functions are stateless and re-entrant.
 *
 * The reference (torchmd/mdgrad, pure Python on PyTorch) has no FFI; each entry point
 * below names the reference op chain (file:line under /root/reference) it replaces.
 * INTEGRATION.md shows the ctypes binding the reference-side maintainer would add.
 */
#ifndef MDGRAD_HIP_H
#define MDGRAD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDG_OK            0
#define MDG_EINVAL       -1   /* bad argument (size / null / unsupported combination) */
#define MDG_ELAUNCH      -2   /* HIP launch error                                     */
#define MDG_ECAPACITY    -3   /* (reported through device flags, see nbr builders)    */

#define MDG_MAX_TERMS     4
#define MDG_MAX_THETA     3   /* per term */
#define MDG_MAX_CHAINS    16

/* pair functional forms -- torchmd/potentials.py */
#define MDG_PAIR_LJ       0   /* 4 eps[(s/r)^p - c (s/r)^q]; theta=(sigma,eps). LennardJones :317-327,
                                 LJFamily :61-73, LennardJones69 :329-339, ExcludedVolume :341-352 (c=0) */
#define MDG_PAIR_MORSE    1   /* ModifiedMorse :75-93; constants a, phi; no parameters */
#define MDG_PAIR_BUCK     2   /* Buck :354-365; theta=(A,B,C) */
#define MDG_PAIR_YUKAWA   3   /* eps exp(-kappa r)/r; theta=(eps,kappa); NOT in the reference */
#define MDG_PAIR_TABLE    4   /* tabulated pair model (user modules such as pairMLP, torchmd/potentials.py:163-206,
                                 or a whole Stack of pair terms with one cutoff): theta = 2 p floats,
                                 theta[2g] = c1(u_g), theta[2g+1] = du * dc1/du(u_g) on the uniform grid
                                 u_g = a + g * phi in u = r^2, where c1(u) = phi'(r)/r; cubic-Hermite
                                 interpolation (force = c1 D; (phi'' - phi'/r)/r^2 = 2 dc1/du).  The adjoint
                                 returns dL/dtheta (the table gradient).  c = fixed-point scale of that
                                 accumulation (a power of two).  Fused small-system kernels only, single
                                 unmasked term, orthorhombic cell. */

typedef struct MdgPairTerm {
    int32_t kind;          /* MDG_PAIR_*                                                    */
    int32_t p, q;          /* LJ-family integer powers (q ignored when c == 0)              */
    float   c;             /* LJ-family attractive coefficient (1 = LJ, 0 = ExcludedVolume) */
    float   a, phi;        /* ModifiedMorse constants                                       */
    float   cutoff;        /* pair kept iff 0 < d^2 < cutoff^2 (topology.py:67)             */
    int32_t theta_off;     /* first parameter of this term inside theta[]                   */
    int32_t n_theta;
    int32_t reserved;
    const uint8_t* mask;   /* optional [N,N] 0/1 selection (index_tuple / ex_pairs,
                              topology.py:15-27,37-53); NULL = all pairs                    */
} MdgPairTerm;

typedef struct MdgTerms {
    int32_t n_terms;
    int32_t n_theta_total;
    MdgPairTerm t[MDG_MAX_TERMS];
} MdgTerms;

/* periodic cell: row vectors h[3][3] and its inverse (host side computes the inverse the
 * way the reference does, `cell.inverse()`, topology.py:59) */
typedef struct MdgCell {
    float h[9];
    float inv[9];
    int32_t diag;          /* 1 when h is diagonal (fast path) */
} MdgCell;

const char* mdg_last_error(void);
int mdg_version(void);

/* ------------------------------------------------------------------------------------
 * K1  neighbour list   (replaces generate_nbr_list, torchmd/topology.py:30-73)
 *
 * Output is a padded per-atom ("ELL") FULL list sorted by neighbour index: row i holds
 * cnt[i] <= max_nbr entries col[i*max_nbr + k] (ascending j, both directions present)
 * and shift[...] = (ox+1) + 3(oy+1) + 9(oz+1), the image flags of the reference's
 * `offsets` for the ordered pair (i,j) (d = x_i - x_j - o.cell).  The reference's
 * half list `nbr_list[P,2]` (i<j, lexicographic) and `offsets[P,3]` are the entries with
 * j > i in row order -- see mdg_nbr_half_from_ell.  *overflow is set to max over rows of
 * the needed count when some row needs more than max_nbr entries (caller re-allocates).
 *
 * mdg_nbr_build_dense: all-pairs minimum image, any (triclinic) cell, O(N^2).
 * mdg_nbr_build_cell : cell list (bin -> sort -> 27-stencil), orthorhombic cells with
 *                      at least 3 bins per side; identical output.  A bin is wider than the
 *                      cutoff by 2^-18 of the box side: nb = floor(L / (cutoff + 2^-18 L)), so a
 *                      box of exactly n cutoffs has n - 1 bins (mdg_nbr_cell_bins: the counts, and
 *                      1 when the cell list takes this cell at this cutoff, else 0).
 * `scratch` for the cell build: int32[ 2*N + 2*ncell_max + 8 ] (see mdg_nbr_cell_scratch).
 */
int mdg_nbr_cell_bins(const MdgCell* cell /*host*/, float cutoff, int32_t* nb /*[3] or NULL*/);
int mdg_nbr_build_dense(const float* pos, int n_atoms, const MdgCell* cell /*host*/,
                        float cutoff, const uint8_t* mask,
                        int32_t* col, int32_t* shift, int32_t* cnt, int max_nbr,
                        int32_t* overflow, void* stream);
/* replica-batched variant: atoms form n_atoms/group independent systems of `group` consecutive
 * atoms sharing one cell; pairs never cross groups; mask (optional) is [group, group]. */
int mdg_nbr_build_dense_groups(const float* pos, int n_atoms, int group, const MdgCell* cell /*host*/,
                               float cutoff, const uint8_t* mask,
                               int32_t* col, int32_t* shift, int32_t* cnt, int max_nbr,
                               int32_t* overflow, void* stream);
int64_t mdg_nbr_cell_scratch(int n_atoms, const MdgCell* cell /*host*/, float cutoff);
int mdg_nbr_build_cell(const float* pos, int n_atoms, const MdgCell* cell /*host*/,
                       float cutoff, const uint8_t* mask,
                       int32_t* col, int32_t* shift, int32_t* cnt, int max_nbr,
                       int32_t* overflow, int32_t* scratch, void* stream);
/* cell list for replica-batched systems (see mdg_nbr_build_dense_groups): every group bins on its own */
int64_t mdg_nbr_cell_scratch_groups(int n_atoms, int group, const MdgCell* cell /*host*/, float cutoff);
int mdg_nbr_build_cell_groups(const float* pos, int n_atoms, int group, const MdgCell* cell /*host*/,
                              float cutoff, const uint8_t* mask,
                              int32_t* col, int32_t* shift, int32_t* cnt, int max_nbr,
                              int32_t* overflow, int32_t* scratch, void* stream);
/* half list in the reference's order: row_base = exclusive scan of per-row (j>i) counts.
 * nbr int64[P,2], offsets f32[P,3]; P must be the value returned in *n_pairs by
 * mdg_nbr_half_count (device int32).  edge_id (optional, int32[N*max_nbr]) receives for
 * every ELL slot the index of its undirected pair in the half list. */
int mdg_nbr_half_count(const int32_t* col, const int32_t* cnt, int n_atoms, int max_nbr,
                       int32_t* row_base /*[N+1]*/, void* stream);
int mdg_nbr_half_fill(const int32_t* col, const int32_t* shift, const int32_t* cnt,
                      const int32_t* row_base, int n_atoms, int max_nbr,
                      int64_t* nbr, float* offsets, int32_t* edge_id, void* stream);
/* Fixed-capacity variant for capture into HIP graphs (no host-side pair count): rows [P, capacity) hold
 * the sentinel pair (-1,-1) -- mdg_edge_diff / mdg_edge_prod return 0 for them -- and the image flag
 * (pad_offset,0,0); n_valid[0] <- min(P, capacity); need[0] <- max(need[0], P) when P > capacity. */
int mdg_nbr_half_fill_padded(const int32_t* col, const int32_t* shift, const int32_t* cnt,
                             const int32_t* row_base, int n_atoms, int max_nbr, int64_t capacity,
                             float pad_offset, int64_t* nbr, float* offsets, int32_t* edge_id,
                             int32_t* n_valid, int32_t* need, void* stream);

/* Verlet reuse of a fixed-capacity list (extension; the reference rebuilds at every call, torchmd/md.py:200-204).  One call per
 * force evaluation, no host synchronisation: the list is searched with list_cutoff = cutoff + skin and kept while every atom
 * stays within half_skin of where it was built -- decided on the device (state[0]); the builder launches return at their
 * first instruction otherwise, so a captured HIP graph replays the same nodes either way.  Consumers re-apply the exact
 * cutoff per pair with the builders' own arithmetic (mdg_edge_geom_masked, mdg_pair_eval_ell_into's recheck bit): the pair
 * set of every evaluation is the one a fresh search at `cutoff` finds.  state int32[4], zero-initialised once (state[3]
 * counts the builds); pos_build [N,3] initialised with NaN; need int32[2] as in the fixed-capacity builders; the remaining
 * buffers are those of mdg_nbr_build_*_groups / mdg_nbr_half_count / mdg_nbr_half_fill_padded, all persistent. */
int mdg_nbr_verlet_rebuild(const float* pos, int n_atoms, int group, const MdgCell* cell /*host*/, float list_cutoff,
                           float half_skin, const uint8_t* mask, int use_cell_list, int32_t* col, int32_t* shift, int32_t* cnt,
                           int max_nbr, int64_t capacity, float pad_offset, int64_t* nbr, float* offsets, int32_t* edge_id,
                           int32_t* n_valid, int32_t* need, float* pos_build, int32_t* state, int32_t* row_base,
                           int32_t* scratch, void* stream);

/* ------------------------------------------------------------------------------------
 * K2-K4  pair energy / gradient / Hessian-vector product over an ELL list
 * (replaces compute_dis + pair form + .sum() and both autograd passes through them:
 *  torchmd/topology.py:5-12, torchmd/interface.py:298-299, torchmd/md.py:227-228,
 *  torchmd/sovlers.py:229-233)
 *
 *   energy[0]      = sum_pairs phi(r)                    (if energy != NULL)
 *   grad[N,3]      = dU/dx                               (if grad   != NULL)  (F = -grad)
 *   gtheta[K]      = dU/dtheta                           (if gtheta != NULL, with grad)
 *   hw[N,3]        = H w                                 (if w != NULL)
 *   gtheta_w[K]    = d(w . dU/dx)/dtheta                 (if w != NULL)
 * One term per call (each term owns its list).  partial: f32 scratch of
 * mdg_pair_partial_size(n_atoms) floats.  Deterministic (no float atomics).
 */
int64_t mdg_pair_partial_size(int n_atoms);
int mdg_pair_eval_ell(const float* pos, int n_atoms, const MdgCell* cell /*host*/,
                      const int32_t* col, const int32_t* shift, const int32_t* cnt, int max_nbr,
                      const MdgPairTerm* term /*host*/, const float* theta,
                      const float* w,
                      float* energy, float* grad, float* gtheta,
                      float* hw, float* gtheta_w,
                      float* partial, void* stream);
/* the same with the per-atom outputs scaled and (accumulate != 0) added onto existing values:
 *   grad = (accumulate ? grad : 0) + out_scale * dU/dx ,  hw likewise -- the force sum of a Stack
 *   (torchmd/interface.py:396-401) without extra launches: F += -dU/dx of this term.  accumulate bit 1 (value 2): the list
 *   was searched with a skin (mdg_nbr_verlet_rebuild); every pair is re-tested with the list builders' own arithmetic
 *   (D = x_j - x_i, reference minimum image, un-contracted d^2 < cutoff^2) before it counts */
int mdg_pair_eval_ell_into(const float* pos, int n_atoms, const MdgCell* cell /*host*/,
                      const int32_t* col, const int32_t* shift, const int32_t* cnt, int max_nbr,
                      const MdgPairTerm* term /*host*/, const float* theta,
                      const float* w,
                      float* energy, float* grad, float* gtheta,
                      float* hw, float* gtheta_w,
                      float* partial, float out_scale, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K5-K7  fused trajectories for small systems (one workgroup per replica, state in LDS,
 * all-pairs minimum image re-evaluated at every force call = the reference's
 * topology_update_freq=1 semantics).
 *
 * forward  (replaces odeint(NH_verlet|verlet): torchmd/sovlers.py:106-127 / 21-40,
 *           torchmd/tinydiffeq.py:56-76, RHS torchmd/md.py:210-240 / 133-150)
 *   ensemble: 0 = NoseHooverChain, 1 = NVE (dv/dt = F, no 1/m: md.py:145-148)
 *   v0,q0 [R,N,3], pv0 [R,C]; t [T] time grid (dt_k = t[k+1]-t[k] in fp32 like the
 *   reference); outputs v_t,q_t [R,T,N,3], pv_t [R,T,C] (frame 0 = inputs).
 *   The force at q_k is evaluated once and reused by the next step (bit-compatible with
 *   the reference's two calls).
 * adjoint  (replaces OdeintAdjointMethod.backward: torchmd/sovlers.py:211-293 with the
 *           backward branches :129-164 / :42-101)
 *   g_* are dL/d(frames) (any may be NULL = zeros); outputs adj_v0,adj_q0 [R,N,3],
 *   adj_pv0 [R,C], adj_theta [R,K] (sum over R on the caller's side; for an MDG_PAIR_TABLE term only that sum is
 *   defined: the wave-per-replica kernels hand the table gradient of eight replicas to the first one's row).
 *   Where the wave-per-replica kernels run (mdg_traj_ring_taken) adj_v0 / adj_q0 may be NULL too -- a caller that wants
 *   adj_theta alone: the launch then leaves out the work that only they need, and, where g_v is NULL, the Hessian-vector
 *   product of the last interval's first evaluation, whose direction is zero (MDG_RING_SKIP_UNREAD=0 in the environment
 *   keeps all of that work; adj_theta is the same bits either way).  Every other route refuses NULL adj_v0 / adj_q0.
 * nonfinite (optional int32[R]): set to 1 for replicas whose state became non-finite.
 */
typedef struct MdgTrajParams {
    int32_t n_rep, n_atoms, n_frames, n_chains;
    int32_t ensemble;
    int32_t block;                 /* 0 = choose */
    float   T;                     /* NHC target temperature (energy units) */
    float   n_dof;                 /* N * dim  (md.py:187) */
    float   Q[MDG_MAX_CHAINS];     /* md.py:191-193 */
} MdgTrajParams;

int mdg_traj_fwd_small(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                       const MdgTerms* terms /*host*/, const float* theta,
                       const float* mass, const float* t_grid,
                       const float* v0, const float* q0, const float* pv0,
                       float* v_t, float* q_t, float* pv_t, int32_t* nonfinite, void* stream);
int mdg_traj_adj_small(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                       const MdgTerms* terms /*host*/, const float* theta,
                       const float* mass, const float* t_grid,
                       const float* v_t, const float* q_t, const float* pv_t,
                       const float* g_v, const float* g_q, const float* g_pv,
                       float* adj_v0, float* adj_q0, float* adj_pv0, float* adj_theta,
                       void* stream);
/* The same two launches keeping the force of every saved frame: f_t is AoS [n_rep][n_frames][n_atoms][3] f32 like q_t
 * (frames 1..n_frames-1 written, frame 0 untouched).  The forward writes it, the adjoint reads it for its first
 * evaluation of each interval instead of rebuilding that force (same bits as f_t = NULL).  Only where the
 * wave-per-replica kernels run, mdg_traj_ring_taken() != 0; elsewhere f_t is ignored.  4 n_rep n_frames n_atoms 3 bytes:
 * 1.06 GB at 16 384 x 50 x 108. */
int mdg_traj_ring_taken(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/);
/* 1 when the one-workgroup-per-replica kernels hold a replica of n_atoms atoms -- with an MDG_PAIR_TABLE term of
 * table_nodes nodes (0: a built-in form) -- in LDS for both the forward and the adjoint launch, else 0: the size rule
 * mdg_traj_fwd_small* / mdg_traj_adj_small* check (the adjoint's state and the table's gradient words are the larger). */
int mdg_traj_small_fits(int n_atoms, int table_nodes);
int mdg_traj_fwd_small_ft(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                          const MdgTerms* terms /*host*/, const float* theta,
                          const float* mass, const float* t_grid,
                          const float* v0, const float* q0, const float* pv0,
                          float* v_t, float* q_t, float* pv_t, float* f_t, int32_t* nonfinite, void* stream);
int mdg_traj_adj_small_ft(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                          const MdgTerms* terms /*host*/, const float* theta,
                          const float* mass, const float* t_grid,
                          const float* v_t, const float* q_t, const float* pv_t, const float* f_t,
                          const float* g_v, const float* g_q, const float* g_pv,
                          float* adj_v0, float* adj_q0, float* adj_pv0, float* adj_theta,
                          void* stream);
/* The same two launches for integrators with topology_update_freq > 1 (torchmd/md.py:200-204: the lists are rebuilt only
 * at the calls whose running count is a multiple of the frequency -- the counter advances on EVERY right-hand-side call,
 * the adjoint's included -- and are stale in between: pair set and image flags frozen at the rebuild positions, no cutoff
 * re-test, i.e. PairPotentials.forward over self.nbr_list / self.offsets, interface.py:298-300).
 *   freq     topology_update_freq;  count0 = the integrator's update_count at the launch's first call.  The forward launch
 *            makes 2 (n_frames - 1) calls (sovlers.py:110-127); the adjoint 3 (n_frames - 1): per interval the dL/dt evaluation
 *            (sovlers.py:258), the first augmented evaluation at the same state, the midpoint evaluation
 *   code     uint16 [n_rep][n_atoms][n_atoms] (mdg_traj_stale_words words), persistent across launches like the reference's
 *            nbr_list / offsets attributes: 0 = no pair, else (term bits << 5) | image code; written at rebuilds
 * Built-in pair forms (any number of terms, masks, any cell) on the generic one-workgroup-per-replica kernels. */
int64_t mdg_traj_stale_words(int n_rep, int n_atoms);
int mdg_traj_fwd_small_stale(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/,
                             const float* theta, const float* mass, const float* t_grid,
                             const float* v0, const float* q0, const float* pv0,
                             float* v_t, float* q_t, float* pv_t, int32_t* nonfinite,
                             int freq, int64_t count0, uint16_t* code, void* stream);
int mdg_traj_adj_small_stale(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/,
                             const float* theta, const float* mass, const float* t_grid,
                             const float* v_t, const float* q_t, const float* pv_t,
                             const float* g_v, const float* g_q, const float* g_pv,
                             float* adj_v0, float* adj_q0, float* adj_pv0, float* adj_theta,
                             int freq, int64_t count0, uint16_t* code, void* stream);

/* Host only, no device needed.  The wave-per-replica kernels round d * inv to the image number with one fused
 * multiply-add where the cell allows it: for the length h and the inverse inv of one axis (the diagonal entries of
 * MdgCell::h / MdgCell::inv) this returns 1 and *inv_fused = a float c (inv or a neighbour within four ulps) for which
 * rint of the EXACT product d c equals rint(fl(d inv)) for every float d with |d inv| < 1.5, or 0 when no such c exists
 * (those cells keep the separately rounded product).  The launches call it themselves; exported for tests. */
int mdg_min_image_fused_inv(float h, float inv, float* inv_fused /*host*/);
/* != 0: a wave-per-replica launch of this system takes the full-ring sweep with the fused minimum image (the ring kernels
 * run, N is even, one unmasked LJ 12-6 / ExcludedVolume(12) term, every axis has a multiplier, MDG_RING_LEAN is not 0);
 * per replica it still needs every atom inside the window of the fast image.  The launches decide with the same code. */
int mdg_traj_ring_fused_image(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/);


/* Fused observable (extension): the radial distribution function of torchmd/observable.py:62-76 evaluated on frames
 * of the trajectory INSIDE the trajectory kernels -- the force sweep already holds every pair distance of a frame, so
 * the forward launch also fills the raw soft histogram (sum over the selected frames of all replicas, the quantity
 * mdg_rdf_fwd_uniform returns for those frames) and the adjoint launch takes g_raw = dL/d(raw) in place of the
 * frame gradients dL/dq_t that mdg_rdf_bwd_uniform would have written to HBM (an additional g_q is still accepted).
 * Available where the wave-per-replica kernels run (one unmasked built-in pair term, orthorhombic cell, N <= 128, and
 * block = 64 or n_rep >= 1024) and for equally spaced centres whose fine grids fit the LDS and start above zero: mdg_traj_rdf_supported() != 0. */
typedef struct MdgRdfFuse {
    const float* mu;               /* device [nbins] centres, equally spaced (GaussianSmearing offsets) */
    int32_t nbins;
    float   coeff;                 /* -0.5 / width^2 */
    float   mu0, spacing;          /* mu[0], mu[1] - mu[0] */
    float   cutoff;                /* pair cutoff of the observable (observable.py:52: r_range end + 0.5) */
    int32_t frame_start, frame_stride;   /* frames frame_start + k frame_stride of every replica */
} MdgRdfFuse;
int mdg_traj_rdf_supported(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                           const MdgTerms* terms /*host*/, const MdgRdfFuse* rdf /*host*/);
int mdg_traj_fwd_small_rdf(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                           const MdgTerms* terms /*host*/, const float* theta,
                           const float* mass, const float* t_grid,
                           const float* v0, const float* q0, const float* pv0,
                           float* v_t, float* q_t, float* pv_t, int32_t* nonfinite,
                           const MdgRdfFuse* rdf /*host*/, float* raw /*[nbins]*/, void* stream);
int mdg_traj_adj_small_rdf(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                           const MdgTerms* terms /*host*/, const float* theta,
                           const float* mass, const float* t_grid,
                           const float* v_t, const float* q_t, const float* pv_t,
                           const float* g_v, const float* g_q, const float* g_pv,
                           float* adj_v0, float* adj_q0, float* adj_pv0, float* adj_theta,
                           const MdgRdfFuse* rdf /*host*/, const float* g_raw /*[nbins]*/, void* stream);
/* the fused-observable launches with the per-frame forces of mdg_traj_fwd_small_ft / mdg_traj_adj_small_ft */
int mdg_traj_fwd_small_rdf_ft(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                              const MdgTerms* terms /*host*/, const float* theta,
                              const float* mass, const float* t_grid,
                              const float* v0, const float* q0, const float* pv0,
                              float* v_t, float* q_t, float* pv_t, float* f_t, int32_t* nonfinite,
                              const MdgRdfFuse* rdf /*host*/, float* raw /*[nbins]*/, void* stream);
int mdg_traj_adj_small_rdf_ft(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                              const MdgTerms* terms /*host*/, const float* theta,
                              const float* mass, const float* t_grid,
                              const float* v_t, const float* q_t, const float* pv_t, const float* f_t,
                              const float* g_v, const float* g_q, const float* g_pv,
                              float* adj_v0, float* adj_q0, float* adj_pv0, float* adj_theta,
                              const MdgRdfFuse* rdf /*host*/, const float* g_raw /*[nbins]*/, void* stream);

/* ------------------------------------------------------------------------------------
 * K5-K7 for systems beyond one workgroup (N <= 32768, NoseHooverChain or NVE): same contract as
 * mdg_traj_fwd_small / mdg_traj_adj_small, three launches per step (forward) / four per adjoint
 * interval, enqueued by a host loop; the neighbour search is fused into the force kernel (per-wave LDS list).
 * Verlet reuse: a search uses the cutoff rc + skin (skin = 12 % of the largest cutoff) and keeps the candidate
 * indices in the workspace; later force evaluations -- forward steps until an atom has moved 0.45 skin from where the
 * list was built (checked on the device every step), and the adjoint's two evaluations per interval -- gather those
 * candidates and re-apply the exact cutoff test, so every evaluation sees the pair set of a fresh search
 * (topology_update_freq = 1, torchmd/sovlers.py:114) while the search itself runs every few steps.
 * (MdgTrajParams.block = -1 switches the reuse off: a fresh search at every evaluation; the adjoint run with the
 * lists reports through flags[5] when that is required.)  mdg_traj_large_list_builds() reports which search served
 * each frame (diagnostics / tests).
 * ws: f32 workspace of mdg_traj_large_workspace() floats, shared by the
 * forward and the adjoint call of one trajectory; flags: int32[8], zeroed by the caller = {neighbour buffer overflow
 * (needed entries), non-finite state, table-gradient range, pair below the table, [4] forward: a stored candidate row
 * overflowed -- call the adjoint with block = -1, [5] adjoint: the stored candidates did not cover an evaluation (row
 * overflow, or a midpoint farther than skin/2 from its frame) -- repeat the adjoint with block = -1}.
 */
int64_t mdg_traj_large_workspace(int n_rep, int n_atoms, int n_frames, int n_theta_total);
int mdg_traj_fwd_large(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                       const MdgTerms* terms /*host*/, const float* theta,
                       const float* mass, const float* t_grid,
                       const float* v0, const float* q0, const float* pv0,
                       float* v_t, float* q_t, float* pv_t, float* ws, int32_t* flags, void* stream);
/* after mdg_traj_fwd_large on `ws` (same sizes): build_of_frame[r][f] (device int32 [n_rep][n_frames]) = the frame whose
 * search produced the candidate list that served frame f; returns 1 (nothing written) when the lists are not kept */
int mdg_traj_large_list_builds(const float* ws, int n_rep, int n_atoms, int n_frames, int n_theta_total,
                               int32_t* build_of_frame, void* stream);
int mdg_traj_adj_large(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/,
                       const MdgTerms* terms /*host*/, const float* theta,
                       const float* mass, const float* t_grid,
                       const float* v_t, const float* q_t, const float* pv_t,
                       const float* g_v, const float* g_q, const float* g_pv,
                       float* adj_v0, float* adj_q0, float* adj_pv0, float* adj_theta,
                       float* ws, int32_t* flags, void* stream);
/* The same two trajectories for integrators with topology_update_freq > 1 (torchmd/md.py:200-204; see mdg_traj_*_small_stale
 * for the call counting: 2 (n_frames - 1) right-hand-side calls per forward launch, 3 (n_frames - 1) per adjoint launch, a
 * rebuild at every call whose running count is a multiple of `freq`, stale pair set + frozen image flags and no cutoff re-test
 * in between, torchmd/interface.py:298-300).  The host loop knows each call's count and launches a searching or a
 * stored-row force kernel accordingly; a forward step whose NEXT first call rebuilds gets one more force launch at the same
 * positions (the two right-hand-side calls that share a state then see different lists).  No Verlet reuse here (the lists ARE
 * the semantics).  Built-in pair forms, any number of terms, masks, any cell, N <= 32 768.
 *   rows  uint32 [mdg_traj_large_stale_words(n_rep, n_atoms)], persistent across launches like the reference's nbr_list /
 *         offsets attributes: per replica and atom 256 entries j | image code << 15 | term bits << 20 in ascending j, then
 *         the int32 counts [n_rep][n_atoms]; flags[0] reports a row overflow as in mdg_traj_fwd_large. */
int64_t mdg_traj_large_stale_words(int n_rep, int n_atoms);
int mdg_traj_fwd_large_stale(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/,
                             const float* theta, const float* mass, const float* t_grid,
                             const float* v0, const float* q0, const float* pv0,
                             float* v_t, float* q_t, float* pv_t, float* ws, int32_t* flags,
                             int freq, int64_t count0, uint32_t* rows, void* stream);
int mdg_traj_adj_large_stale(const MdgTrajParams* prm /*host*/, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/,
                             const float* theta, const float* mass, const float* t_grid,
                             const float* v_t, const float* q_t, const float* pv_t,
                             const float* g_v, const float* g_q, const float* g_pv,
                             float* adj_v0, float* adj_q0, float* adj_pv0, float* adj_theta,
                             float* ws, int32_t* flags, int freq, int64_t count0, uint32_t* rows, void* stream);

/* ------------------------------------------------------------------------------------
 * K8  soft-histogram RDF  (replaces rdf.forward and its autograd backward:
 *     torchmd/observable.py:62-76 with GaussianSmearing nff/nn/layers.py:14-31)
 *   xyz [F,N,3]; pairs i<j with 0 < d < cutoff (min image) over all frames;
 *   raw[k] = sum exp(coeff (d - mu_k)^2), mu_k = mu0 + k*dmu, k < nbins.
 *   fwd writes raw[nbins] (normalisation / volume factors are cheap host-side torch ops).
 *   bwd: given g_raw[nbins] = dL/draw, writes g_xyz [F,N,3].
 *   partial: f32 scratch of mdg_rdf_partial_size(...) floats.
 */
int64_t mdg_rdf_partial_size(int n_frames, int n_atoms, int nbins);
int mdg_rdf_fwd(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell /*host*/,
                float cutoff, const uint8_t* mask, const float* mu /*[nbins]*/, float coeff,
                int nbins, float* raw, float* partial, void* stream);
/* same, with the caller's guarantee that mu is an equally spaced grid (mu_k = mu[0] + k*spacing, as
 * torch.linspace gives).  Forward, in order of preference (mdg_rdf_fwd_variant tells which one a shape takes):
 *   FINE    >= 1024 frames of 64 .. 1024 atoms whose fine grid fits the LDS: pairs counted on a fine integer
 *           histogram, smeared onto the centres once;
 *   HALF    >= 1024 frames, <= 4096 atoms, s*spacing in [0.8455, 1.5] and ~120 bins at most: one wave per frame,
 *           one lane per pair, half-width lane-private LDS columns, eight waves per workgroup;
 *   LANE    >= 1024 frames, <= 4096 atoms, s*spacing >= 0.405: the same with full-width columns (reach 5 or 11 bins);
 *   BLOCK8  s*spacing <= 1 and >= 16 bins: persistent workgroups, 8 bins per thread with the Gaussian recurrence;
 *   DIRECT  everything else, and every call of mdg_rdf_fwd: one bin per thread.
 * (s = sqrt(-coeff log2 e).)  More than 512 bins are refused.  Backward (mdg_rdf_bwd_variant):
 *   ATOM    fewer than 1024 frames or more than 4096 atoms: 16 lanes per (frame, atom);
 *   TABLE   s*spacing in [0.465, 1] and at most 4096 table nodes: one wave per frame, dL/dd from a cubic-Hermite table;
 *   FRAME   otherwise: one wave per frame, bin recurrence over 6 or 11 bins each side (s*spacing >= 0.465) or the
 *           direct sum; refused when a frame does not fit the LDS.
 * A scratch allocation that fails is MDG_ELAUNCH in both directions. */
#define MDG_RDF_FWD_DIRECT 0
#define MDG_RDF_FWD_BLOCK8 1
#define MDG_RDF_FWD_LANE   2
#define MDG_RDF_FWD_HALF   3
#define MDG_RDF_FWD_FINE   4
#define MDG_RDF_BWD_ATOM   0
#define MDG_RDF_BWD_TABLE  1
#define MDG_RDF_BWD_FRAME  2
#define MDG_RDF_PLAN_INFO  6
/* Host only, no launch: the variant the shape takes (spacing <= 0: no guarantee on mu), or -1 where the launch would
 * refuse it.  info, when not NULL, receives MDG_RDF_PLAN_INFO words: {reach in bins, waves per workgroup, workgroups,
 * dynamic LDS bytes, row stride of the LDS coordinates, forward: 1 when that stride is the compile-time 128 /
 * backward: cells of the derivative table}. */
int mdg_rdf_fwd_variant(int n_frames, int n_atoms, int nbins, float spacing, float coeff, int diag, int masked,
                        int32_t* info);
int mdg_rdf_bwd_variant(int n_frames, int n_atoms, int nbins, float spacing, float coeff, int diag, int masked,
                        int32_t* info);
/* Host only: the fine integer grid of these centres -- the one the FINE variant, mdg_rdf_fwd_ell and mdg_rdf_fwd_cell count
 * on: `bins` bins (0: it does not fit) of width h from mu[0] - reach -- and the nodes per centre spacing of the backward's
 * derivative table; any pointer may be NULL.  0, or -1 where the centres have no such grid (spacing <= 0, coeff >= 0). */
int mdg_rdf_fine_grid(float spacing, float coeff, int nbins, int32_t* bins, float* h, float* reach, int32_t* table_sub);
int mdg_rdf_fwd_uniform(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell /*host*/,
                        float cutoff, const uint8_t* mask, const float* mu, float spacing, float coeff,
                        int nbins, float* raw, float* partial, void* stream);
int mdg_rdf_bwd(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell /*host*/,
                float cutoff, const uint8_t* mask, const float* mu, float coeff, int nbins,
                const float* g_raw, float* g_xyz, void* stream);
/* Soft histogram of a system given as a per-atom neighbour list (large systems, few frames; frames stacked as groups of
 * the list): every pair (slot neighbour index above the atom's) counted once on a fine integer grid, then smeared onto
 * the equally spaced centres -- the pair search of torchmd/observable.py:64-66 is the list build.  The gradient is a
 * tabulated pair force (mdg_pair_eval_ell with an MDG_PAIR_TABLE term built from g_raw). */
int mdg_rdf_ell_supported(float spacing, float coeff, int nbins);
int mdg_rdf_fwd_ell(const float* pos, int64_t n_atoms_total, const MdgCell* cell /*host*/, const int32_t* col,
                    const int32_t* shift, const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff,
                    int nbins, float* raw, void* stream);
/* The same observable straight from the cell bins, without materialising a neighbour list (the list build costs more
 * than the histogram): per frame, positions sorted by (bin, atom index); a wave per atom walks the 27-bin stencil and
 * counts every pair once on the fine integer grid (forward), or sums the tabulated pair force of
 * phi(d) = sum_k g_k exp(coeff (d - mu_k)^2) (backward: term/theta = the MDG_PAIR_TABLE built from dL/d raw, as for
 * mdg_pair_eval_ell; g_xyz [F][N][3] = dL/dxyz).  Orthorhombic cells of >= 3 bins per side, bins counted as
 * mdg_nbr_cell_bins counts them (wider than `cutoff` by 2^-18 of the side), N <= 32 768
 * (mdg_rdf_cell_supported); cutoff = the list cutoff (>= the reach of the fine grid).  scratch: int32 words of
 * mdg_rdf_cell_scratch(), 16-byte aligned, filled by the forward call and read by the backward call of the same frames.
 * Replaces torchmd/observable.py:62-76 (generate_nbr_list + GaussianSmearing(...).sum(0)) and its autograd transpose. */
int mdg_rdf_cell_supported(int n_atoms, const MdgCell* cell /*host*/, float cutoff);
int64_t mdg_rdf_cell_scratch(int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff);
int mdg_rdf_fwd_cell(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff,
                     const float* mu, float spacing, float coeff, int nbins, float* raw, int32_t* scratch, void* stream);
int mdg_rdf_bwd_cell(int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff,
                     const MdgPairTerm* term /*host*/, const float* theta, const int32_t* scratch, float* g_xyz,
                     void* stream);
/* backward with the same equally-spaced-centres guarantee (mdg_rdf_bwd makes no assumption on mu). */
int mdg_rdf_bwd_uniform(const float* xyz, int n_frames, int n_atoms, const MdgCell* cell /*host*/,
                        float cutoff, const uint8_t* mask, const float* mu, float spacing, float coeff,
                        int nbins, const float* g_raw, float* g_xyz, void* stream);

/* ------------------------------------------------------------------------------------
 * K10  graph gather/scatter for the SchNet continuous-filter convolution
 * (replaces the index / scatter_add_ chains of nff/nn/models/schnet.py:142,
 *  nff/nn/modules.py:564-571, nff/nn/graphconv.py:43-53 and their autograd transposes).
 * nbr = int64 [E,2] half list (i<j); col/eid/cnt = ELL list with undirected edge ids
 * (mdg_nbr_half_fill).  Feature matrices are row-major fp32.
 *   mdg_edge_diff    out[e,c] = x[i_e,c] - x[j_e,c]
 *   mdg_edge_scatter out[n,c] = sum_{slots s of n} (+/-) g[eid_s,c]     (+ when n is i_e)
 *   mdg_cfconv_agg   out[n,f] = sum_{slots s of n} h[col_s,f] * W[eid_s,f]
 *   mdg_edge_prod    out[e,f] = a[i_e,f] b[j_e,f] + a[j_e,f] b[i_e,f]
 */
int mdg_edge_diff(const float* x, const int64_t* nbr, int64_t n_edges, int n_feat, float* out, void* stream);
int mdg_edge_scatter(const float* g, const int32_t* col, const int32_t* eid, const int32_t* cnt,
                     int n_atoms, int max_nbr, int n_feat, float* out, void* stream);
int mdg_cfconv_agg(const float* h, const float* W, const int32_t* col, const int32_t* eid,
                   const int32_t* cnt, int n_atoms, int max_nbr, int n_feat, float* out, void* stream);
int mdg_edge_prod(const float* a, const float* b, const int64_t* nbr, int64_t n_edges, int n_feat,
                  float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * K9  continuous-filter generator on the matrix cores (fp32-input MFMA, exact f32)
 * (replaces GaussianSmearing -> Dense(G,G) -> shifted_softplus -> Dense(G,F):
 *  nff/nn/modules.py:531-541, nff/nn/layers.py:14-31,86-134, nff/nn/activations.py:5-11)
 *   d [E] distances; mu, width [G] (coeff_k = -0.5 / width_k^2); W1 [G,G], b1 [G], W2 [F,G],
 *   b2 [F] in torch.nn.Linear layout ([out,in]); out [E,F].   G <= 64.
 */
int mdg_cfconv_filter(const float* d, int64_t n_edges, const float* mu, const float* width, int n_gauss,
                      const float* W1, const float* b1, const float* W2, const float* b2,
                      int n_filters, float* out, void* stream);

/* bf16-operand variant (v_mfma_f32_16x16x32_bf16, fp32 accumulate / bias / output). */
int mdg_cfconv_filter_bf16(const float* d, int64_t n_edges, const float* mu, const float* width, int n_gauss,
                           const float* W1, const float* b1, const float* W2, const float* b2,
                           int n_filters, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Velocity observables as single fused passes over v_t [T, N, 3]:
 *   mdg_vacf_fwd     out[t] = mean over frames s, atoms, components of v[s+t] v[s], t = 0 .. n_lags-1
 *                    (torchmd/observable.py:153-163 vacf.forward; n_dof_per_frame = N * 3)
 *   mdg_vacf_bwd     g_v = d(sum_t g_out[t] out[t]) / dv
 *   mdg_temperature  out[f] = sum_n m_n |v_n|^2 / n_dof   (torchmd/thermo.py:57-66 on every frame; n_dof = N * dim)
 * workspace: mdg_vacf_workspace(n_lags) floats.
 */
int64_t mdg_vacf_workspace(int n_lags);
int mdg_vacf_fwd(const float* v, int n_frames, int64_t n_dof_per_frame, int n_lags, float* out, float* workspace,
                 void* stream);
int mdg_vacf_bwd(const float* v, const float* g_out, int n_frames, int64_t n_dof_per_frame, int n_lags, float* g_v,
                 void* stream);
int mdg_temperature(const float* v, const float* mass, int n_frames, int n_atoms, float n_dof, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * K9 + K10 fused: the whole SchNet interaction block on the MD path, nothing edge-sized in HBM
 * (replaces SchNetConv.message/aggregate -- nff/nn/modules.py:531-541,564-571, nff/nn/graphconv.py:43-53,
 *  the distance line nff/nn/models/schnet.py:142 -- and what autograd / double autograd derive from them for
 *  the force -dU/dx and for the adjoint's d(w.F)/dx, d(w.F)/dtheta, torchmd/sovlers.py:229-233).
 * Filter network: mu, coef [G] (coef_k = -0.5 / width_k^2), W1 [G,G], b1 [G], W2 [F,G], b2 [F] in
 * torch.nn.Linear layout.  G <= 64; F <= 128, a multiple of 4 (F <= 64) or 8 (mdg_cfconv_supported).
 *
 *   mdg_edge_geom      d_e = |x_i - x_j - o_e|, uhat_e; with w: dd_e = uhat_e . (w_i - w_j), ddel_e = w_i - w_j
 *   mdg_cfconv_fwd     m[n] = sum_{slots s of n} h[col_s] (.) W(d_s)                        (dd == NULL)
 *                      md[n] = sum_s h[col_s] (.) dW/dd(d_s) dd_s + hd[col_s] (.) W(d_s)    (tangent; hd nullable)
 *                      hsum[n] = sum_s h[col_s], hdsum likewise (nullable; feed the bias gradient of Dense2)
 *                      Symmetric in the adjacency: called with (h, hd) := (mdb, mb) it returns the adjoints
 *                      (hdb, hb) of (hd, h) in the reverse sweep.
 *   mdg_cfconv_bwd     with Wdb_e = mdb_i h_j + mdb_j h_i and (dual sweep, mb != NULL)
 *                      Wb_e = mb_i h_j + mb_j h_i + mdb_i hd_j + mdb_j hd_i:
 *                        dd_b[e] += d(Wdb_e . Wd_e)/d(dd_e)        d_b[e] += d(Wdb_e . Wd_e + Wb_e . W_e)/d(d_e)
 *                        gW1, gb1, gW2 <- gradients of sum_e (Wdb_e . Wd_e + Wb_e . W_e)   (gW1 != NULL; dual only)
 *                      Called with mdb := dU/dm and mb == NULL it is the plain reverse sweep: dd_b[e] += dU/dd_e.
 *                      workspace: mdg_cfconv_bwd_workspace() floats when gW1 is requested.
 *   mdg_edge_geom_bwd  force[n] = -sum_s sgn_s dd_b uhat ;  dwf[n] = -sum_s sgn_s [d_b uhat + dd_b/d (ddel - dd uhat)]
 *                      (d_b nullable: force only)
 */
typedef struct {
    const float* mu;
    const float* coef;
    const float* W1;
    const float* b1;
    const float* W2;
    const float* b2;
    int32_t n_gauss, n_filters;
} MdgFilterNet;               /* host struct of DEVICE pointers */

int mdg_cfconv_supported(int n_gauss, int n_filters);
int mdg_edge_geom(const float* x, const float* w, const int64_t* nbr, const float* offsets, int64_t n_edges,
                  float* d, float* uhat, float* dd, float* ddel, void* stream);
/* mdg_edge_geom for a list searched with a skin: pairs that fail the builders' cutoff test at the current positions get
 * d = -1 (and dd = 0) and are skipped by the cfconv kernels like padding */
int mdg_edge_geom_masked(const float* x, const float* w, const int64_t* nbr, const float* offsets, int64_t n_edges,
                         const MdgCell* cell /*host*/, float cutoff, float* d, float* uhat, float* dd, float* ddel, void* stream);
/* mdg_edge_geom (cell == NULL) / mdg_edge_geom_masked and the zero fill of zero_n floats at `zero` (nullable) in one launch */
int mdg_edge_geom_prepare(const float* x, const float* w, const int64_t* nbr, const float* offsets, int64_t n_edges,
                          const MdgCell* cell /*host, nullable*/, float cutoff, float* d, float* uhat, float* dd, float* ddel,
                          float* zero, int64_t zero_n, void* stream);
int mdg_edge_geom_bwd(const float* d_b, const float* dd_b, const float* d, const float* dd, const float* uhat,
                      const float* ddel, const int32_t* col, const int32_t* eid, const int32_t* cnt,
                      int n_atoms, int max_nbr, float* force, float* dwf, void* stream);
int mdg_cfconv_fwd(const MdgFilterNet* net /*host*/, const float* d, const float* dd, const float* h, const float* hd,
                   const int32_t* col, const int32_t* eid, const int32_t* cnt, int n_atoms, int max_nbr,
                   float* m, float* md, float* hsum, float* hdsum, void* stream);
/* bf16-operand MFMA variant of mdg_cfconv_fwd (v_mfma_f32_16x16x32_bf16; fp32 accumulate, biases, activation,
 * products with the node rows and sums): BASELINE config #5's "bf16 cfconv MFMA" on the trajectory path. */
int mdg_cfconv_fwd_bf16(const MdgFilterNet* net /*host*/, const float* d, const float* dd, const float* h,
                        const float* hd, const int32_t* col, const int32_t* eid, const int32_t* cnt, int n_atoms,
                        int max_nbr, float* m, float* md, float* hsum, float* hdsum, void* stream);
int64_t mdg_cfconv_bwd_workspace(int n_gauss, int n_filters, int64_t n_edges);
int mdg_cfconv_bwd(const MdgFilterNet* net /*host*/, const float* d, const float* dd, const int64_t* nbr,
                   int64_t n_edges, const float* h, const float* hd, const float* mb, const float* mdb,
                   float* d_b, float* dd_b, float* gW1, float* gb1, float* gW2, float* workspace,
                   const int32_t* n_valid /*device, nullable: real rows of a capacity-padded list*/, void* stream);
/* bf16-operand MFMA variant of mdg_cfconv_bwd (v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x16_bf16; everything else fp32):
 * the reverse half of BASELINE config #5's "bf16 cfconv MFMA, full fwd + adjoint".  Same arguments and workspace. */
int mdg_cfconv_bwd_bf16(const MdgFilterNet* net /*host*/, const float* d, const float* dd, const int64_t* nbr,
                        int64_t n_edges, const float* h, const float* hd, const float* mb, const float* mdb,
                        float* d_b, float* dd_b, float* gW1, float* gb1, float* gW2, float* workspace,
                        const int32_t* n_valid, void* stream);
/* either of the two with the gradients of the radial basis as well (GaussianSmearing(trainable=True), nff/nn/layers.py:34-83:
 * `offsets` and `width` are parameters): gmu[G] = d/d(mu_k), gcoef[G] = d/d(coef_k) of the same scalar; the caller chains
 * coef = -0.5 / width^2.  bf16 != 0: bf16 MFMA operands. */
int mdg_cfconv_bwd_smear(const MdgFilterNet* net /*host*/, const float* d, const float* dd, const int64_t* nbr,
                         int64_t n_edges, const float* h, const float* hd, const float* mb, const float* mdb,
                         float* d_b, float* dd_b, float* gW1, float* gb1, float* gW2, float* gmu, float* gcoef,
                         float* workspace, const int32_t* n_valid, int bf16, void* stream);

/* "rows16": the bf16 variants over bf16 MIRRORS of the node matrices the kernels GATHER per edge (h, hd and, in the reverse
 * sweep, mb, mdb): [n_atoms, n_filters] bf16, dense rows, round-to-nearest-even copies of the f32 matrices (mdg_row_chain
 * writes them next to its f32 outputs, mdg_rows_to_bf16 makes one of any f32 matrix).  A gathered row is then one 16-byte
 * load per lane instead of two and half the cache lines; it widens exactly and every product, sum and output stays f32.
 * This is a PRECISION OPTION of its own on top of the bf16 MFMA operands (the gathered features carry 8 significant bits
 * into the products; nff/nn/modules.py:564-571 multiplies f32 features) -- callers opt in explicitly
 * (SchNet.node_rows_bf16, bench.py --bf16-rows) and tests/test_gpu_schnet_rows16.py states its tolerance.
 * Layers of more than 64 filters (mdg_cfconv_rows16_supported).  Outputs, workspace and the other arguments as in
 * mdg_cfconv_fwd_bf16 / mdg_cfconv_bwd_smear (gmu = gcoef = NULL: no basis gradients). */
int mdg_cfconv_rows16_supported(int n_gauss, int n_filters);
int mdg_cfconv_fwd_rows16(const MdgFilterNet* net /*host*/, const float* d, const float* dd, const uint16_t* h16,
                          const uint16_t* hd16, const int32_t* col, const int32_t* eid, const int32_t* cnt, int n_atoms,
                          int max_nbr, float* m, float* md, float* hsum, float* hdsum, void* stream);
int mdg_cfconv_bwd_rows16(const MdgFilterNet* net /*host*/, const float* d, const float* dd, const int64_t* nbr,
                          int64_t n_edges, int n_atoms, const uint16_t* h16, const uint16_t* hd16, const uint16_t* mb16,
                          const uint16_t* mdb16, float* d_b, float* dd_b, float* gW1, float* gb1, float* gW2, float* gmu,
                          float* gcoef, float* workspace, const int32_t* n_valid, void* stream);
/* The G-wide stash of the filter network (round 6): its first Dense layer -- Gaussians, a = g W1^T + b1, s = ssp(a) and, with
 * dd, the tangent sd = sigmoid(a) a_dot (nff/nn/modules.py:531-541, layers 0-2 of message_edge_filter) -- ONCE per undirected
 * edge and evaluation, as [n_edges][W] bf16 rows (W = mdg_cfconv_stash_width(n_gauss): 32 or 64; 64 bytes per edge and
 * quantity at W = 32), zero rows for pairs beyond the cutoff (d = -1) and padding.  mdg_cfconv_fwd_stashed is
 * mdg_cfconv_fwd_bf16 / _rows16 reading the second layer's operands from it instead of recomputing them per directed slot
 * (every edge from both ends, in each of the sweeps of an evaluation): the same bf16 operands, so bitwise the same outputs.
 * d may be NULL when n_gauss + 2 <= W (the second layer's bias then rides in two spare k columns). */
int mdg_cfconv_stash_width(int n_gauss);
int mdg_cfconv_filter_stash(const MdgFilterNet* net /*host*/, const float* d, const float* dd /*nullable*/, int64_t n_edges,
                            const int32_t* n_valid /*device, nullable*/, uint16_t* st_s, uint16_t* st_sd /*with dd*/, void* stream);
int mdg_cfconv_fwd_stashed(const MdgFilterNet* net /*host*/, const uint16_t* st_s, const uint16_t* st_sd /*nullable: no tangent*/,
                           const float* d /*see above*/, const void* h, const void* hd /*nullable*/, const int32_t* col,
                           const int32_t* eid, const int32_t* cnt, int n_atoms, int max_nbr, float* m, float* md /*with st_sd*/,
                           int rows16, void* stream);
/* The reverse sweep with parameter gradients, every option in one entry.  flags: MDG_CFCONV_BF16 (bf16 MFMA operands as
 * mdg_cfconv_bwd_bf16) | MDG_CFCONV_ROWS16 (with BF16: h, hd, mb, mdb are bf16 mirrors, n_atoms rows each).  gb2[n_filters]
 * (nullable; needs mdg_cfconv_bias_column(n_gauss)): d/d b2 of the same scalar, sum over the edges of the filter output's
 * adjoint rows -- it falls out of a spare padded column of the first filter layer whose activation is pinned to 1
 * (csrc/cfconv_fused.hip: B2COL_BIAS), so the caller needs neither the neighbour sums of mdg_cfconv_fwd (hsum / hdsum) nor a
 * reduction over atoms for it (nff/nn/modules.py:531-541: the bias of Dense(n_gaussians -> n_filters)' second layer).
 * gmu / gcoef (nullable, together) as in mdg_cfconv_bwd_smear. */
enum { MDG_CFCONV_BF16 = 1, MDG_CFCONV_ROWS16 = 2 };
int mdg_cfconv_bias_column(int n_gauss);
int mdg_cfconv_bwd_theta(const MdgFilterNet* net /*host*/, const float* d, const float* dd, const int64_t* nbr,
                         int64_t n_edges, int n_atoms, const void* h, const void* hd, const void* mb, const void* mdb,
                         float* d_b, float* dd_b, float* gW1, float* gb1, float* gW2, float* gb2, float* gmu, float* gcoef,
                         float* workspace, const int32_t* n_valid, int flags, void* stream);
/* dst[r, c] = bf16(src[r * src_stride + c]), dense [n_rows, n_cols] bf16 (n_cols, src_stride multiples of 4) */
int mdg_rows_to_bf16(const float* src, int64_t n_rows, int n_cols, int src_stride, uint16_t* dst, void* stream);

/* ------------------------------------------------------------------------------------
 * K11/K12  node-level Dense layers with fused epilogues on the f32 MFMA
 * (replaces nff/nn/layers.py:86-134 Dense + nff/nn/activations.py:5-11 on [N, .] node features: message_node_filter,
 *  the update MLP + residual nff/nn/modules.py:543-547 / schnet.py:149-151, the readout's first Linear, and the
 *  transposed products of the hand-derived reverse sweeps):
 *     z0 = x0 B + bias0 ;  out0 = act(z0) * mul0 + res0 ;  sig0 = sigmoid(z0)            (act = 1: shifted softplus)
 *     z1 = x1 B          ;  out1 = act'(z0) z1 + res1                                     (x1 nullable)
 *  B[k][m] = W[m*k_dim + k] (trans = 0, torch.nn.Linear layout) or W[k*m_dim + m] (trans = 1).  Any k: layers wider than
 *  256 inputs run as k-slabs of 256 that hand their partial sums on through out0 / out1.
 */
int mdg_dense(const float* W, int trans, int act, int n_rows, int k, int m,
              const float* x0, const float* bias0, const float* mul0, const float* res0, float* out0, float* sig0,
              const float* x1, const float* res1, float* out1, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused elementwise / row-reduction pieces of the hand-derived SchNet passes (each replaces a chain of
 * PyTorch elementwise ops; nff/nn/layers.py:14-31, nff/nn/activations.py:5-11 and their derivatives):
 *   mdg_smear        g = exp(c_k (d - mu_k)^2), phi = 2 c_k (d - mu_k)              [E,G]
 *   mdg_ssp          s = softplus(a) - ln 2 (, sa = sigmoid(a))
 *   mdg_mul_row      o = x * y (* r[row])
 *   mdg_ssp_dual_bwd xdb = sa sdb ; xb = sa (1 - sa) xd sdb + sa sb
 *   mdg_smear_bwd    d_b[e] += sum_k (...), dd_b[e] += sum_k (...)   (see csrc/elem.hip)
 */
int mdg_smear(const float* d, const float* mu, const float* c, int64_t n_edges, int n_gauss, float* g, float* phi,
              void* stream);
int mdg_ssp(const float* a, int64_t n, float* s, float* sa, void* stream);
int mdg_mul_row(const float* x, const float* y, const float* r, int64_t n_rows, int n_cols, float* o, void* stream);
int mdg_ssp_dual_bwd(const float* sa, const float* xd, const float* sdb, const float* sb, int64_t n, float* xdb,
                     float* xb, void* stream);
/* the same with the tangent given as t_dot = sa * x_dot:  xdb = sa sdb ; xb = (1 - sa) t_dot sdb + sa sb */
int mdg_ssp_dual_bwd_t(const float* sa, const float* td, const float* sdb, const float* sb, int64_t n, float* xdb,
                       float* xb, void* stream);
/* head of the reverse sweeps through the readout U = sum_i L2 . ssp(y_i) + l2 (nff/nn/modules.py:761-809, schnet.py:155-158):
 * ydb = sy * L2 ; yb = (1 - sy) * syd * L2, with sy = sigmoid(y) and syd = sy * y_dot [n_rows, n_cols], L2 [n_cols];
 * syd = yb = NULL: first-order pass */
int mdg_readout_head(const float* sy, const float* syd, const float* L2, int64_t n_rows, int n_cols, float* ydb, float* yb,
                     void* stream);
int mdg_smear_bwd(const float* gdb, const float* gb, const float* g, const float* phi, const float* dd,
                  const float* c, int64_t n_edges, int n_gauss, float* d_b, float* dd_b, void* stream);

/* ------------------------------------------------------------------------------------
 * Tall-skinny contraction C[M,N] = A[E,M]^T B[E,N] (split-K on the f32 MFMA, ordered reduction):
 * the weight gradients of edge-wise Dense layers in the adjoint's parameter vjp (autograd of
 * nff/nn/layers.py:86-134 on [E, .] inputs).  workspace: mdg_atb_workspace() floats.
 */
int64_t mdg_atb_workspace(int64_t n_rows, int m, int n);
int mdg_atb(const float* A, const float* B, int64_t n_rows, int m, int n, float* C, float* workspace,
            void* stream);
/* C = A^T B + A2^T B2 (same shapes; A2 = B2 = NULL: mdg_atb): primal + tangent halves of a weight gradient at once */
int mdg_atb2(const float* A, const float* B, const float* A2, const float* B2, int64_t n_rows, int m, int n, float* C,
             float* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * K13  a CHAIN of such Dense layers in one launch (csrc/rowchain.hip): between two continuous-filter convolutions every
 * operation of a SchNet block is local to one atom's feature row -- update MLP + residual (nff/nn/modules.py:543-547,
 * nff/nn/models/schnet.py:149-151), the next block's message_node_filter, the readout (nff/nn/modules.py:761-809) -- and so
 * is the stretch of the hand-derived reverse sweeps from the readout head back to the adjoint of the last aggregation.  A
 * workgroup owns 16 rows and walks the stages; a stage's outputs stay on chip as the next stage's input and are copied to
 * the global buffers the caller names.  Per stage (x = in0 / in1 when given, else the previous stage's outputs):
 *     z0 = x0 B + bias ; z1 = x1 B                        B[k][m] = W[m*K + k] (trans = 0) or W[k*M + m] (trans = 1)
 *     act = 1:          out0 = ssp(z0), sig = sigmoid(z0), out1 = sig z1
 *     MDG_CHAIN_MUL     out0 *= aux0[row, m]
 *     MDG_CHAIN_HEAD    (act = 1) pre0 = out0, pre1 = out1 ; out0 = sig aux0[m] ; out1 = (1 - sig) pre1 aux0[m]
 *     MDG_CHAIN_SSP_BWD out0 = s z0 ; out1 = (1 - s) td z0 + s z1         (s = aux0[row, m], td = aux1[row, m])
 *     then out0 += res0[row, m], out1 += res1[row, m]; out0_h / out1_h (when given) receive the same values rounded to bf16
 * dual = 0: only the "0" operands are touched.  aux0 / aux1 / res may be buffers an EARLIER stage of the same call wrote
 * with the same width M (same owner thread); any other aliasing between a stage's outputs and a later stage's inputs is
 * not allowed.  Widths 1..MDG_CHAIN_MAX_WIDTH, 1..MDG_CHAIN_MAX_STAGES stages.
 * flags: MDG_CHAIN_DUAL (= the former `dual` argument: 0 / 1) | MDG_CHAIN_X3: the stage products as three bf16 MFMAs on
 * operands split into bf16 head + bf16 remainder (x_h w_h + x_h w_l + x_l w_h, f32 accumulate: ~1e-5 relative per product
 * instead of 6e-8, 3/16 of the matrix time) -- the companion of the rows16 precision option, honoured by the compiled
 * n_atom_basis = 64 chains and ignored (f32 products) by every other list.  MDG_CHAIN_X6 (instead): THREE exact bf16 pieces
 * per operand and the six piece products that matter -- the accuracy of the f32 matrix instruction (1.8e-7 of sum |terms|,
 * tools/micro/split_mfma.hip) at 3/8 of its issue time; honoured by every compiled chain.
 */
#define MDG_CHAIN_MAX_STAGES 8
#define MDG_CHAIN_MAX_WIDTH 512
enum { MDG_CHAIN_NONE = 0, MDG_CHAIN_MUL = 1, MDG_CHAIN_HEAD = 2, MDG_CHAIN_SSP_BWD = 3 };
enum { MDG_CHAIN_DUAL = 1, MDG_CHAIN_X3 = 2, MDG_CHAIN_X6 = 4 };
typedef struct {
    const float* W;
    const float* bias;
    const float* in0;
    const float* in1;
    const float* res0;
    const float* res1;
    const float* aux0;
    const float* aux1;
    float* out0;
    float* out1;
    float* sig;
    float* pre0;
    float* pre1;
    uint16_t* out0_h;   /* nullable: bf16 mirrors [n_rows, M] of out0 / out1 (the rows16 kernels' inputs), written with them */
    uint16_t* out1_h;
    int32_t K, M, trans, act, mode, pad_;
} MdgChainStage;
int mdg_row_chain(const MdgChainStage* stages, int n_stages, int n_rows, int flags, void* stream);

/* ------------------------------------------------------------------------------------
 * All parameter-gradient reductions of one SchNet adjoint evaluation in two launches (csrc/gradjobs.hip): what double
 * autograd accumulates into the .grad of the Dense weights / biases and the embedding of nff/nn/modules.py:514-575 and
 * nff/nn/models/schnet.py:113-171 while it differentiates w.F (torchmd/sovlers.py:229-233), times the interval weight of
 * sovlers.py:160.  A job is one reduction over `rows` atoms:
 *   MDG_GRAD_ATB     out[m,n] = A[rows,m]^T B[rows,n] (+ A2^T B2); row r of the result goes to destination row
 *                    row_map[r] when row_map != NULL (rows of the embedding table), else r
 *   MDG_GRAD_COLSUM  out[m]   = sum_rows A (.* B) (+ A2 (.* B2))            (B, B2 optional, together)
 *   MDG_GRAD_AXPY    out[m]   = A (+ A2)                                     (already reduced: cfconv_bwd's gW1, gb1, gW2)
 * and lands at flat[out_off ...]:  flat = (accumulate ? flat : 0) + alpha * (t ? t[*idx] - t[*idx - 1] : 1) * out, with the
 * time grid t and the frame index idx on the device (a captured HIP graph advances idx itself).  Fixed-order sums, no
 * atomics.  workspace: mdg_grad_jobs_workspace() floats.  At most MDG_GRAD_JOBS_MAX jobs per call.
 */
#define MDG_GRAD_JOBS_MAX 32
enum { MDG_GRAD_ATB = 0, MDG_GRAD_COLSUM = 1, MDG_GRAD_AXPY = 2 };
typedef struct {
    const float* A;
    const float* B;
    const float* A2;
    const float* B2;
    const int64_t* row_map;
    int64_t rows;
    int32_t m, n;
    int32_t kind, pad_;
    int64_t out_off;
} MdgGradJob;
int64_t mdg_grad_jobs_workspace(const MdgGradJob* jobs, int n_jobs);
int mdg_grad_jobs(const MdgGradJob* jobs, int n_jobs, float* flat, float alpha, const float* t, const int64_t* idx,
                  int accumulate, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * One SchNet evaluation per call (csrc/schnet_eval.hip, round 6): what GNNPotentials.forward + compute_grad
 * (torchmd/interface.py:86-136, torchmd/md.py:23-31: F = -dU/dx by autograd through nff/nn/models/schnet.py:113-171) and the
 * adjoint's vector-Jacobian product of it (torchmd/sovlers.py:229-233: d(w.F)/dx, d(w.F)/dtheta by double autograd) compute,
 * as the hand-derived sweeps of mdgrad_amd/nn/analytic.py -- primal (+ tangent along w), turn at the readout, reverse -- with
 * every launch of the evaluation (edge geometry, the fused interaction-block kernels, the row chains of the node-level layers,
 * the batched parameter-gradient reductions) enqueued by one C++ loop on `stream`.  The caller describes the network and the
 * topology with DEVICE pointers and hands over one workspace of mdg_schnet_workspace() floats; nothing is allocated inside.
 *
 *   layer[i]   one interaction block (nff/nn/modules.py:514-575): Gaussian basis + filter network (`filt`), message_node_filter
 *              (Wn [F, A], bn), update MLP (U1 [A, F], c1; U2 [A, A], c2), torch.nn.Linear layout.  bf16 / bf16_rev: bf16 MFMA
 *              operands in the forward-type / reverse sweeps of the filter network; rows16: the block's kernels gather bf16
 *              mirrors of the node rows (mdg_cfconv_*_rows16); b2col: d/d b2 from the spare filter column (mdg_cfconv_bwd_theta).
 *              off_*: offset of each parameter in the flat parameter-gradient vector (tinydiffeq.py:106-108 order).
 *   readout    L1 [H, A], l1 [H], L2 [H] (nff/nn/utils.py:56-75: Linear, shifted_softplus, Linear(H -> 1)).
 *   r0, h0     embedding rows atom_embed.weight[z] [N, A] and the first block's filtered rows Wn r0 + bn [N, F] (neither depends
 *              on the positions: persistent buffers of the caller); h0_16: bf16 mirror of h0 (first block rows16).
 *   onehot, uniq, n_species    [N, S] one-hot of the species and the S embedding rows in use (gradient of atom_embed.weight).
 *   topology   half list nbr [E, 2] + image offsets [E, 3] and the per-atom rows col / eid / cnt of the same list
 *              (mdg_nbr_*; capacity-padded lists: n_valid = device count of real rows).  masked: the list was searched with a
 *              skin -- pairs beyond `cutoff` in `cell` at the current positions are skipped (mdg_edge_geom_masked).
 * Results are bitwise those of the launch-by-launch sequence (tests/test_gpu_schnet_plan.py).
 */
#define MDG_SCHNET_MAX_LAYERS 8
typedef struct {
    MdgFilterNet filt;
    const float *Wn, *bn, *U1, *c1, *U2, *c2;
    int64_t off_W1, off_b1, off_W2, off_b2, off_Wn, off_bn, off_U1, off_c1, off_U2, off_c2;
    int32_t bf16, bf16_rev, rows16, b2col;
} MdgSchnetLayer;
typedef struct {
    int32_t n_atoms, n_layers, n_atom_basis, n_readout;
    MdgSchnetLayer layer[MDG_SCHNET_MAX_LAYERS];
    const float *L1, *l1, *L2;
    int64_t off_L1, off_l1, off_L2, off_embed;
    const float *r0, *h0;
    const uint16_t* h0_16;
    const float* onehot;
    const int64_t* uniq;
    int32_t n_species, masked;
    const int64_t* nbr;
    const float* offsets;
    int64_t n_edges;
    const int32_t *col, *eid, *cnt;
    const int32_t* n_valid;
    int32_t max_nbr;
    float cutoff;
    MdgCell cell;
    float* ws;
    int64_t ws_floats;
    int32_t stash, chain_x3;  /* chain_x3: MDG_CHAIN_X3 or MDG_CHAIN_X6 (or 0), handed to mdg_row_chain with every node-level chain.  stash != 0: blocks with bf16 operands run mdg_cfconv_filter_stash once per evaluation and the
                                 stashed forward-type sweeps (mdg_cfconv_fwd_stashed): same results, fewer instructions */
} MdgSchnetPlan;              /* host struct of DEVICE pointers */
int64_t mdg_schnet_plan_sizeof(void);      /* sizeof(MdgSchnetPlan): bindings in other languages check their layout against it */
/* floats of workspace: dual = 0 for mdg_schnet_force, dual = 1 for mdg_schnet_force_vjp (theta != 0: with parameter gradients) */
int64_t mdg_schnet_workspace(const MdgSchnetPlan* plan /*host*/, int dual, int theta);
/* force [N, 3] = -dU/dx.  energy_colsum [H] (nullable): column sums of the readout's activations; U = L2 . colsum + N l2 */
int mdg_schnet_force(const MdgSchnetPlan* plan /*host*/, const float* x, float* force, float* energy_colsum, void* stream);
/* force, dwf [N, 3] = d(w.F)/dx and, theta_flat != NULL, theta_flat += alpha * (t ? t[*idx] - t[*idx - 1] : 1) * dU_dot/dtheta
 * (callers pass alpha = -1: w.F = -U_dot; t / idx: the device-side interval weight of sovlers.py:160, together or NULL) */
int mdg_schnet_force_vjp(const MdgSchnetPlan* plan /*host*/, const float* x, const float* w, float* force, float* dwf,
                         float* theta_flat, float alpha, const float* t, const int64_t* idx, float* energy_colsum, void* stream);

/* ------------------------------------------------------------------------------------
 * Nose-Hoover-chain algebra of the generic (non-fused) integrator path as single launches
 * (replaces the elementwise/reduction ops of NoseHooverChain.forward after the force,
 *  torchmd/md.py:221-240, and the thermostat part of its vjp).
 * State of R stacked replicas: v, f, lv, lq [R*n, 3]; pv, lp [R, C]; mass [R*n]; Q [C].
 *   mdg_nhc_rhs:  a = (f - pv0 m v / Q0) / m ;  dpv = bath right-hand side (KE per replica)
 *   mdg_nhc_vjp:  Gv = -(pv0/Q0) lv + lq + 2 m v lp0 ;  Gp = lam^T d(bath rhs)/d pv - (lv.v)/Q0 e0
 */
int mdg_nhc_rhs(const float* v, const float* f, const float* pv, const float* mass, const float* Q,
                const float* T /*device, [1]*/, float n_dof, int n_rep, int n_atoms, int n_chains, float* a,
                float* dpv, void* stream);
int mdg_nhc_vjp(const float* v, const float* pv, const float* lv, const float* lq, const float* lp,
                const float* mass, const float* Q, int n_rep, int n_atoms, int n_chains, float* Gv,
                float* Gp, void* stream);
/* Whole half-steps of the generic NH-Verlet path (interactions that are not pair-fusable, e.g. SchNet) as single
 * launches: torchmd/sovlers.py:110-127 (forward) and :129-164 with :253-288 (adjoint interval), the force / force-vjp
 * evaluations in between stay separate calls.  Time-major frames [T, R*n, 3] / [T, R, C]; idx: device int64[1], the
 * step k (forward) or frame i (adjoint) -- a captured HIP graph advances it itself; dt = t[k+1] - t[k] is read on the
 * device.
 *   mdg_nhv_kick     dv_h = 1/2 a dt, dp_h = 1/2 b dt, qn = q + (v + dv_h) dt           (rhs at (v, q, pv), cached force f)
 *   mdg_nhv_finish   v += dv_h + 1/2 a1 dt, pv += dp_h + 1/2 b1 dt, q = qn, f = fn ; frame k+1 stored
 *   mdg_nhv_adj_pre  (v, q, pv) <- frame i ;  w = lam_v / m
 *   mdg_nhv_adj_mid  vh = v - a hh, qm = q + vh h, pm = pv - b hh, lam_h = lam + G0 hh, wh = lam_h_v / m
 *   mdg_nhv_adj_end  lam += G1 h + dL/dy_{i-1}
 * A replica's elements are cut over several workgroups; `scratch` (mdg_nhv_scratch_floats(n_rep, n_atoms) floats,
 * zeroed ONCE by the caller, reusable by every launch of the same shape on one stream) carries the per-workgroup
 * partial sums of the kinetic energy / <lam_v, v> and a ticket per replica; the result does not depend on the order
 * the workgroups finish in.  advance != 0 (mdg_nhv_finish / mdg_nhv_adj_end): the launch also moves the counter, idx[0] <- k + 1
 * resp. i - 1, once every workgroup has read the old value -- no separate increment launch per step. */
int64_t mdg_nhv_scratch_floats(int n_rep, int n_atoms);
int mdg_nhv_kick(const float* v, const float* q, const float* pv, const float* f, const float* mass, const float* Q,
                 const float* T, float n_dof, const float* t, const int64_t* idx, int n_rep, int n_atoms, int n_chains,
                 float* dv_h, float* dp_h, float* qn, float* scratch, void* stream);
int mdg_nhv_finish(float* v, float* q, float* pv, float* f, const float* dv_h, const float* dp_h, const float* qn,
                   const float* fn, const float* mass, const float* Q, const float* T, float n_dof, const float* t,
                   int64_t* idx, int advance, int n_rep, int n_atoms, int n_chains, float* out_v, float* out_q, float* out_pv,
                   float* scratch, void* stream);
int mdg_nhv_adj_pre(const float* v_t, const float* q_t, const float* pv_t, const float* lv, const float* mass,
                    const int64_t* idx, int n_rep, int n_atoms, int n_chains, float* v, float* q, float* pv, float* w,
                    void* stream);
int mdg_nhv_adj_mid(const float* v, const float* q, const float* pv, const float* lv, const float* lq, const float* lp,
                    const float* f, const float* dwf, const float* mass, const float* Q, const float* T, float n_dof,
                    const float* t, const int64_t* idx, int n_rep, int n_atoms, int n_chains, float* vh, float* qm, float* pm,
                    float* lvh, float* lqh, float* lph, float* wh, float* scratch, void* stream);
int mdg_nhv_adj_end(const float* vh, const float* pm, const float* lvh, const float* lqh, const float* lph, const float* dwf,
                    const float* mass, const float* Q, const float* t, int64_t* idx, int advance, const float* g_v,
                    const float* g_q, const float* g_pv, int n_rep, int n_atoms, int n_chains, float* lv, float* lq,
                    float* lp, float* scratch, void* stream);
/* Langevin dynamics (BAOAB) on the same generic path (csrc/langevin.hip): one step as two launches around the ONE force
 * evaluation, one adjoint interval as one launch between two force-vjp evaluations.  State of M = R*n stacked atoms:
 * v, q, f, lv, lq, w [M, 3]; mass [M]; time-major frames [T, M, 3]; idx as above; gamma, T: device float[1]; rng: device
 * int64[2] = (seed, step0) -- a captured HIP graph follows changes of all of them.
 *   h = t[k+1] - t[k], c1 = exp(-gamma h), c2 = sqrt(-expm1(-2 gamma h))
 *   mdg_lgv_kick      v1 = v + (h/2) f/m, q1 = q + (h/2) v1, v2 = c1 v1 + c2 sqrt(T/m) xi, qn = q1 + (h/2) v2
 *   mdg_lgv_finish    v = v2 + (h/2) fn/m, q = qn, f = fn ; frame k+1 stored
 *   mdg_lgv_adj_pre   q <- frame i ;  w = (h/2) lam_v / m                                       (h = t[i] - t[i-1])
 *   mdg_lgv_adj_step  given f = F(q_i), dwf = H(q_i) w:  lam_q += dwf ; lam_v += (h/2) lam_q ;
 *                     gpart[workgroup] += sum lam_v h (sqrt(T/m) xi / c2 - v2), v2 = v_i - (h/2) f/m   (want_gamma) ;
 *                     lam_v = c1 lam_v + (h/2) lam_q ; w = (h/2) lam_v / m ; lam += g[i-1] ;
 *                     w += (h'/2) lam_v / m, h' = t[i-1] - t[i-2] (i >= 2) ; q <- frame i-1
 *   mdg_lgv_gamma_sum out[0] = the mdg_lgv_blocks(M) slots of gpart added in slot order (zero gpart before a sweep)
 *   mdg_lgv_noise     xi [M, 3] of step rng[1] + step_off
 * xi: Philox4x32-10, key = (seed lo, seed hi), counter = (atom row, step lo, step hi, 0), step = step0 + k (adjoint:
 * step0 + i - 1); u_j = ((x_j >> 9) + 1/2) 2^-23; xi = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3), r0 = sqrt(-2 ln u0),
 * r1 = sqrt(-2 ln u2).  ticket: one zeroed uint32 shared by the launches of one stream (handed back at zero); advance != 0
 * (mdg_lgv_finish / mdg_lgv_adj_step): idx[0] <- k + 1 resp. i - 1 once every workgroup has read the old value.  Bitwise
 * reproducible: no floating-point atomics. */
int mdg_lgv_blocks(int n_total);
int mdg_lgv_noise(const int64_t* rng, int64_t step_off, int n_total, float* xi, void* stream);
int mdg_lgv_kick(const float* v, const float* q, const float* f, const float* mass, const float* gamma, const float* T,
                 const float* t, const int64_t* idx, const int64_t* rng, int n_total, float* v2, float* qn, void* stream);
int mdg_lgv_finish(float* v, float* q, float* f, const float* v2, const float* qn, const float* fn, const float* mass,
                   const float* t, int64_t* idx, int advance, int n_total, float* out_v, float* out_q, uint32_t* ticket,
                   void* stream);
int mdg_lgv_adj_pre(const float* q_t, const float* lv, const float* mass, const float* t, const int64_t* idx, int n_total,
                    float* q, float* w, void* stream);
int mdg_lgv_adj_step(const float* v_t, const float* q_t, const float* f, const float* dwf, const float* mass,
                     const float* gamma, const float* T, const float* t, int64_t* idx, int advance, const int64_t* rng,
                     const float* g_v, const float* g_q, int want_gamma, int n_total, float* lv, float* lq, float* q, float* w,
                     float* gpart, uint32_t* ticket, void* stream);
int mdg_lgv_gamma_sum(const float* gpart, int n_total, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * K14 bond-angle distribution  (replaces angle_distribution.forward and its autograd backward:
 *      torchmd/observable.py:120-151, compute_angle :166-179, generate_angle_list torchmd/topology.py:83-122;
 *      csrc/adf.hip)
 *   pos [n_frames * n_atoms, 3]; col / cnt: the ELL list of K1 over those rows (frames = groups of n_atoms, col holds row
 *   indices); the cell must be diagonal.  Every ordered triplet (i, j, k) of one frame with (i, j) and (j, k) listed pairs and
 *   k != i is counted: theta at centre j between u = x_i - x_j and v = x_k - x_j, both re-imaged with topology.get_offsets.
 *   raw[b] = sum exp(coeff (theta - mu_b)^2), mu_b = mu[0] + b * spacing, b < nbins <= 4096; centres farther than
 *   5.3 / sqrt(-coeff log2 e) from theta are dropped (<= 2^-28 of a peak term each).
 *   fwd: raw[nbins] (NaN if an angle is not finite); scratch: int64 words of mdg_adf_partial_size(), bitwise reproducible.
 *   bwd: given g_raw[nbins] = dL/draw, writes g_xyz [n_frames * n_atoms, 3]; triplets with |u x v| <= 2^-20 |u| |v|
 *   contribute zero (the symmetric subgradient at theta = 0, pi).  Bitwise reproducible, no atomics.
 */
int64_t mdg_adf_partial_size(int n_frames, int n_atoms, int max_nbr, int nbins);
int mdg_adf_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff, const int32_t* col,
                const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff, int nbins, float* raw,
                int64_t* scratch, void* stream);
int mdg_adf_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff, const int32_t* col,
                const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff, int nbins,
                const float* g_raw, float* g_xyz, void* stream);

/* K35  the bond-angle histogram of every frame on its own (mdgrad_amd/observable.py angle_distribution.per_frame; csrc/adf.hip):
 *      the rows whose sum over the frames K14 returns -- same list, triplets, re-imaging, atan2 angle, weight 2, reach and
 *      recurrence.
 *   fwd: raw [n_frames, nbins].  A workgroup per frame; its contributions are summed as fixed-point integers in LDS and written
 *        straight to raw[f, :]: bitwise reproducible, no global atomics, no scratch.  The scale comes from the triplet bound of
 *        one frame, n_atoms max_nbr (max_nbr - 1) / 2.  A non-finite angle makes the row of its frame NaN and no other.
 *   bwd: given g_raw [n_frames, nbins], writes g_xyz [n_frames * n_atoms, 3] = d(sum_fb g_raw raw)/d pos; atom-centric, every
 *        thread reads the g_raw row of its own frame, the degenerate-triplet rule of K14, no atomics.  A frame whose g_raw row
 *        is zero gets zeros.
 */
int mdg_adf_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff, const int32_t* col,
                       const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff, int nbins, float* raw,
                       void* stream);
int mdg_adf_frames_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff, const int32_t* col,
                       const int32_t* cnt, int max_nbr, const float* mu, float spacing, float coeff, int nbins,
                       const float* g_raw, float* g_xyz, void* stream);

/* ------------------------------------------------------------------------------------
 * K15  pair virial of every frame and its gradient: the configurational part of the pressure
 *      P = (sum_i m_i |v_i|^2 + W) / (dim V)  (mdgrad_amd/thermo.py Pressure; the reference's sketch, torchmd/thermo.py:17-54,
 *      uses undefined names and does not run; csrc/virial.hip)
 *   pos [n_frames, n_atoms, 3]; the cell must be diagonal; terms: 1..MDG_MAX_TERMS built-in forms (MDG_PAIR_LJ .. MDG_PAIR_YUKAWA),
 *   each with its own cutoff and optional [n_atoms, n_atoms] mask, parameters packed in term order (theta_off = running sum).
 *   W[f] = - sum_terms sum_pairs r phi'(r) over the pair set PairPotentials sums the energy over: i < j, the strict +-1/2
 *   minimum image of topology.py:59-64, 0 < d^2 < cutoff^2 (un-contracted d^2 like the list builders), the term's mask.
 *   W = -dU/ds at s = 1 for x -> s x, L -> s L with the pair set held fixed.
 *   fwd: W[n_frames].
 *   bwd: given gW[n_frames] = dL/dW, writes g_pos [n_frames, n_atoms, 3] = gW_f sum_j (phi' + r phi'') (x_j - x_i) / r and
 *        g_theta[n_theta_total] = - sum_f gW_f sum_pairs r dphi'/dtheta (nullable without parameters).
 *   List-free all-pairs sweeps (a wave per frame up to 128 atoms, a workgroup per frame up to 1024, 256 x 256 tiles up to
 *   32 768); n_frames < 2^24.  workspace: mdg_virial_workspace() floats, shared by both calls.  Fixed-order sums, no
 *   floating-point atomics: bitwise reproducible.
 */
int64_t mdg_virial_workspace(int n_frames, int n_atoms, int n_theta_total);
int mdg_virial_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/,
                   const float* theta, float* W, float* workspace, void* stream);
int mdg_virial_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/,
                   const float* theta, const float* gW, float* g_pos, float* g_theta, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * K16  static structure factor S(k) of every frame and its gradient (mdgrad_amd/observable.py structure_factor; the
 *      reference has none, the definition is this project's; csrc/sk.hip)
 *   pos [n_frames, n_atoms, 3]; the cell must be diagonal, lengths L.  kvec int32 [n_vecs, 3]: integer wave vectors n,
 *   k(n) = 2 pi (nx / Lx, ny / Ly, nz / Lz), |n_d| <= 1024, sorted by bin; seg int32 [n_bins + 1]: ascending offsets of the bins'
 *   segments in kvec (seg[0] = 0, seg[n_bins] = n_vecs; an empty bin repeats an offset).  weights: nullable [n_atoms] (null =
 *   unit weights); norm = sum_i w_i^2 (n_atoms for unit weights), formed by the caller.
 *     rho_f(k) = sum_i w_i exp(i k.x_fi)     S_f(k) = |rho_f(k)|^2 / norm     S[f, b] = mean of S_f(k) over bin b (0 when empty)
 *   fwd: S [n_frames, n_bins].
 *   bwd: given gS [n_frames, n_bins] = dL/dS, writes g_pos [n_frames, n_atoms, 3]
 *        = sum_k (gS[f, b(k)] / count_b) (2 w_i / norm) (Im rho cos k.x - Re rho sin k.x) k;  rho is recomputed per frame.
 *   Phases are reduced in turns per axis before sine and cosine (positions many cells outside the box lose nothing).
 *   List-free phase sums (a wave per frame up to 128 atoms, a workgroup per frame up to 1024, atom-block x vector-chunk tiles up
 *   to 32 768); n_frames < 2^24, 1 <= n_vecs <= 65 536, 1 <= n_bins <= 1024.  workspace: mdg_sk_workspace() floats, shared by
 *   both calls.  Fixed-order sums: bitwise reproducible.
 */
int64_t mdg_sk_workspace(int n_frames, int n_atoms, int n_vecs);
int mdg_sk_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const float* weights, float norm,
               const int32_t* kvec, int n_vecs, const int32_t* seg, int n_bins, float* S, float* workspace, void* stream);
int mdg_sk_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const float* weights, float norm,
               const int32_t* kvec, int n_vecs, const int32_t* seg, int n_bins, const float* gS, float* g_pos, float* workspace,
               void* stream);

/* ------------------------------------------------------------------------------------
 * K17  mean-squared displacement of a trajectory over all lags, its fourth moment and their gradient
 *      (mdgrad_amd/observable.py msd; the reference has none, the definition is this project's; csrc/msd.hip)
 *   x [n_batch, n_frames, n_cols, 3], one continuous (unwrapped) trajectory per batch entry; the n_cols columns are
 *   n_cols / group replicas of `group` atoms each, and replica c / group of batch b owns output row
 *   b * (n_cols / group) + c / group.  weights: nullable [group], w_i >= 0 and not all zero (null = unit weights).
 *   With T = n_frames, s = origin_stride and the origins O_tau = {t0 = 0, s, 2 s, ... : t0 + tau < T}, per row
 *     M_p[tau] = 1 / (|O_tau| sum_i w_i)  sum_{t0 in O_tau} sum_i w_i |x_i(t0 + tau) - x_i(t0)|^p ,  tau = 0 .. n_lags - 1
 *   All three components, no cell, no re-imaging.  M_p[0] is exactly 0.
 *   fwd: out2 [rows, n_lags] (p = 2) and, unless null, out4 [rows, n_lags] (p = 4).
 *   bwd: given g2 [rows, n_lags] = dL/dM_2 and g4 (nullable) = dL/dM_4, writes every element of gx [n_batch, n_frames,
 *        n_cols, 3] once:  gx_i(t) = w_i sum_tau [ (t - tau in O_tau) f(x_t - x_{t-tau}) - (t in O_tau, t + tau < T)
 *        f(x_{t+tau} - x_t) ],  f(d) = (2 g2_tau + 4 g4_tau |d|^2) d / (|O_tau| sum w).
 *   Every position is read from device memory once: a workgroup walks through time with a ring of frames of its atom tile
 *   in LDS and takes all lags from it.  1 <= n_lags <= min(n_frames, 1024), origin_stride >= 1, n_cols % group == 0.
 *   workspace: mdg_msd_workspace() floats, enough for either call.  Fixed-order sums, no floating-point atomics: bitwise
 *   reproducible.  mdg_msd_tile_atoms / _window / _max_lags: the forward's atom tile (16), frame window (16) and the lag limit.
 */
int64_t mdg_msd_workspace(int n_batch, int n_cols, int group, int n_lags, int fourth);
int mdg_msd_fwd(const float* x, int n_batch, int n_frames, int n_cols, int group, const float* weights, int n_lags,
                int origin_stride, float* out2, float* out4, float* workspace, void* stream);
int mdg_msd_bwd(const float* x, int n_batch, int n_frames, int n_cols, int group, const float* weights, int n_lags,
                int origin_stride, const float* g2, const float* g4, float* gx, float* workspace, void* stream);
int mdg_msd_tile_atoms(void);
int mdg_msd_window(void);
int mdg_msd_max_lags(void);

/* ------------------------------------------------------------------------------------
 * K18  intermediate scattering functions of a trajectory over all lags, coherent F(k,t) and self F_s(k,t), and their gradient
 *      (mdgrad_amd/observable.py intermediate_scattering; the reference has none, the definition is this project's;
 *      csrc/isf.hip)
 *   x [n_batch, n_frames, n_cols, 3]; the n_cols columns are n_cols / group replicas of `group` atoms each.  One call takes the
 *   replicas rep0 .. rep0 + n_reps - 1 of every batch entry (callers chunk the rows that way to bound the workspace); replica r
 *   of batch b owns output row b * n_reps + (r - rep0).  cell: diagonal, positive lengths L.  weights: nullable [group]
 *   (null = unit weights), norm = W2 = sum_i w_i^2 > 0.  kvec int32 [n_vecs, 3] and seg int32 [n_bins + 1] as in K16.
 *   kind: 0 coherent, 1 self.  With T = n_frames, s = origin_stride, O_tau = {t0 = 0, s, 2 s, ... : t0 + tau < T}, per row
 *     rho(k, t)   = sum_i w_i exp(i k.x_i(t))
 *     F(k, tau)   = 1 / (|O_tau| W2)  sum_{t0 in O_tau} Re[ rho(k, t0 + tau) conj rho(k, t0) ]
 *     F_s(k, tau) = 1 / (|O_tau| W2)  sum_{t0 in O_tau} sum_i w_i^2 cos( k.(x_i(t0 + tau) - x_i(t0)) ) ,  tau = 0 .. n_lags - 1
 *   and F[b, tau] = the mean over the vectors of bin b (0 for an empty bin).
 *   fwd: F [rows, n_bins, n_lags].
 *   bwd: given gF [rows, n_bins, n_lags] = dL/dF, writes every element of gx that belongs to the call's replicas once (the
 *        other columns are not touched); an atom of weight 0 gets exactly 0.
 *   Coherent: rho of every (frame, vector) goes to the workspace, the origin sums run in double.  Self: one sine / cosine pair
 *   per (frame, atom, vector); a workgroup walks through time with a ring of phasors in LDS and takes all lags from it.
 *   1 <= n_lags <= min(n_frames, mdg_isf_max_lags()), origin_stride >= 1, n_cols % group == 0, 1 <= n_vecs <= 65 536,
 *   1 <= n_bins <= 1024, coherent: group <= 32 768.  workspace: mdg_isf_workspace(kind, n_batch * n_reps, ...) floats (never
 *   null: pass one float where it returns 0), enough for either call:
 *     self      rows * n_vecs * n_lags * ceil(group / 16)
 *     coherent  2 * rows * n_vecs * (n_frames * ceil(group / 1024) + max(n_lags, n_frames))
 *   Fixed-order sums, no floating-point atomics: bitwise reproducible, and a row's result does not depend on which other rows
 *   share its call.  mdg_isf_max_lags / _tile_atoms / _window: the lag limit and the self forward's atom tile and frame window.
 */
int64_t mdg_isf_workspace(int kind, int64_t n_rows, int n_frames, int group, int n_vecs, int n_lags);
int mdg_isf_fwd(int kind, const float* x, int n_batch, int n_frames, int n_cols, int group, int rep0, int n_reps,
                const MdgCell* cell /*host*/, const float* weights, double norm, const int32_t* kvec, int n_vecs,
                const int32_t* seg, int n_bins, int n_lags, int origin_stride, float* F, float* workspace, void* stream);
int mdg_isf_bwd(int kind, const float* x, int n_batch, int n_frames, int n_cols, int group, int rep0, int n_reps,
                const MdgCell* cell /*host*/, const float* weights, double norm, const int32_t* kvec, int n_vecs,
                const int32_t* seg, int n_bins, int n_lags, int origin_stride, const float* gF, float* gx, float* workspace,
                void* stream);
int mdg_isf_max_lags(void);
int mdg_isf_tile_atoms(void);
int mdg_isf_window(void);

/* ------------------------------------------------------------------------------------
 * K19  dihedral (torsion) terms over a static table of quadruples: the torsion energy with force, Hessian-vector product
 *      and parameter gradients, the per-term angles of many frames, and their periodic soft histogram
 *      (mdgrad_amd/interface.py DihedralPotentials, mdgrad_amd/observable.py Dihedrals / dihedral_distribution; the cosine is
 *      torchmd/observable.py:181-197 compute_dihe, the energy the "multiharmonic" form of nff/nn/modules.py:253-257;
 *      csrc/dihedral.hip)
 *   top int32 [n_terms, 4] rows (i, j, k, l); cell_len host float[3], the diagonal of the cell.
 *     b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k, each re-imaged with topology.get_offsets (-[b >= L/2] + [b < -L/2]);
 *     n1 = b1 x b2, n2 = b2 x b3;  cos phi = n1.n2 / sqrt(|n1|^2 |n2|^2);  phi = atan2(|b2| b1.n2, n1.n2) in (-pi, pi] (IUPAC)
 *     U = sum_{m = 0..4} coeff[type, m] cos^m phi
 *   Degenerate terms: |n1|^2 <= eps^2 |b1|^2 |b2|^2 or |n2|^2 <= eps^2 |b2|^2 |b3|^2, eps = 2^-20 (K14's threshold), are skipped
 *   everywhere: zero energy, force, H w, parameter gradient, histogram weight and gradient; phi = cos phi = 0, zero gradient.
 *   inc_ptr int32 [n_atoms + 1], inc int32 [4 n_terms]: the incidence list of every atom as in f4 (entries 4 * term + role,
 *   ascending per atom -- the order the per-atom sums run in).  No atomics on floats anywhere: bitwise reproducible.
 *
 *   mdg_dihedral_eval  mirrors mdg_bonded_eval (one launch): coeff device float [n_types, 5], type nullable device int32
 *     [n_terms] with entries in [0, n_types) (null = all type 0); w nullable [n_atoms, 3], required for hw;
 *     e_atom nullable [n_atoms] (energy of the terms whose FIRST atom this is); grad, hw nullable [n_atoms, 3]:
 *     grad = (accumulate ? grad : 0) + out_scale * dU/dx, hw likewise with H w;  c_term, cd_term nullable [n_terms]:
 *     cos phi of every term (MDG_DIHEDRAL_SKIPPED = 2 for a skipped term) and its directional derivative w.grad(cos phi)
 *     (0 without w).
 *   mdg_dihedral_coeff_grad  from c_term / cd_term: g_u [n_types, 5] = dU/dcoeff[s, m] = sum_{t of type s} c_t^m and
 *     g_w [n_types, 5] = d(w.dU/dx)/dcoeff[s, m] = sum_t m c_t^(m-1) cd_t (either nullable), in a fixed order.
 *   mdg_dihedral_phi_fwd  pos [n_frames, n_atoms, 3] -> phi, cosphi [n_frames, n_terms] (either nullable).
 *   mdg_dihedral_phi_bwd  given g_phi and / or g_cos [n_frames, n_terms] (the other null), writes g_xyz [n_frames, n_atoms, 3];
 *     d phi/dx in the Blondel-Karplus form, finite at phi = 0 and +-pi.
 *   mdg_dihedral_hist_fwd  raw[b] = sum_i exp(-1/2 (wrap(phi_i - mu_b) / width)^2) over phi [n], mu_b = -pi + (b + 1/2) 2 pi / nbins,
 *     wrap onto [-pi, pi) (nearest image only), 1 <= nbins <= 4096, 0 < width <= 0.5; centres farther than
 *     5.3 width sqrt(2 ln 2) from phi are dropped (<= 2^-28 of a peak term each, as K14).  cosphi nullable [n]: with it, an entry
 *     with phi == 0 and cosphi == 0 is a skipped term and carries no weight.  NaN if an angle is not finite.  scratch: int64
 *     words of mdg_dihedral_hist_scratch().
 *   mdg_dihedral_hist_bwd  given g_raw [nbins], writes g_phi [n] = sum_b g_raw[b] d raw[b] / d phi_i.
 */
#define MDG_DIHEDRAL_SKIPPED 2.0f
int mdg_dihedral_eval(const float* pos, int n_atoms, const float* cell_len /*host*/, const int32_t* top, int n_terms,
                      const float* coeff, const int32_t* type, int n_types, const int32_t* inc_ptr, const int32_t* inc,
                      const float* w, float* e_atom, float* grad, float* hw, float* c_term, float* cd_term, float out_scale,
                      int accumulate, void* stream);
int mdg_dihedral_coeff_grad(const float* c_term, const float* cd_term, const int32_t* type, int n_terms, int n_types,
                            float* g_u, float* g_w, void* stream);
int mdg_dihedral_phi_fwd(const float* pos, int n_frames, int n_atoms, const float* cell_len /*host*/, const int32_t* top,
                         int n_terms, float* phi, float* cosphi, void* stream);
int mdg_dihedral_phi_bwd(const float* pos, int n_frames, int n_atoms, const float* cell_len /*host*/, const int32_t* top,
                         int n_terms, const int32_t* inc_ptr, const int32_t* inc, const float* g_phi, const float* g_cos,
                         float* g_xyz, void* stream);
int64_t mdg_dihedral_hist_scratch(int64_t n, int nbins);
int mdg_dihedral_hist_fwd(const float* phi, const float* cosphi, int64_t n, int nbins, float width, float* raw,
                          int64_t* scratch, void* stream);
int mdg_dihedral_hist_bwd(const float* phi, const float* cosphi, int64_t n, int nbins, float width, const float* g_raw,
                          float* g_phi, void* stream);

/* ------------------------------------------------------------------------------------
 * K20  damped shifted-force Coulomb sum over the per-atom (ELL) list with one charge per atom (Wolf et al. 1999; Fennell and
 *      Gezelter 2006; mdgrad_amd/interface.py CoulombPotentials, csrc/coulomb.hip).  With E(r) = erfc(alpha r) and
 *      G(r) = g0 exp(-alpha^2 r^2), g0 = 2 alpha / sqrt(pi):
 *        psi(r) = E/r - c0 + c1 (r - rc)      psi' = -E/r^2 - G/r + c1      psi'' = 2E/r^3 + 2G/r^2 + 2 alpha^2 G
 *        U = conversion [ 1/2 sum_i sum_{j in row(i)} q_i q_j psi(r_ij) - self_s sum_i q_i^2 ]
 *      MdgCoulombConsts is prepared by the host in double (c0, c1: 0 or the values that make psi / psi' vanish at rc; self_s:
 *      c0/2 + alpha/sqrt(pi), or 0).  alpha == 0 takes E = 1, G = 0 without evaluating either function.
 *   mdg_coulomb_eval  laid out like mdg_pair_eval_ell_into (same list, same `accumulate` bits: 1 = add onto grad / hw,
 *     2 = the list was searched with a skin, re-apply the exact cutoff test per pair; same out_scale), q device float [n_atoms].
 *     w nullable [n_atoms, 3], required for hw / potw.  Outputs, each nullable:
 *       energy [1] = U (needs `partial`, mdg_coulomb_partial_size() floats; fixed-order block partials + a finish kernel)
 *       grad [n_atoms, 3] = (accumulate & 1 ? grad : 0) + out_scale dU/dx,  hw likewise with H w
 *       pot [n_atoms]  = sum_j q_j psi(r_ij)                      (dU/dq_i = conversion (pot_i - 2 self_s q_i))
 *       potw [n_atoms] = sum_j q_j psi'(r_ij) rhat_ij.(w_i - w_j)  (d(w.dU/dx)/dq_i = conversion potw_i)
 *     No atomics: bitwise reproducible.
 *   mdg_coulomb_charge_reduce  out[p] = sum of val[i] over the atoms with slot(i) == p, p in [0, n_slots), in a fixed order:
 *     slot(i) = types[i % group] (types device int32 [group], n_slots = number of types) or i % group (types null,
 *     n_slots = group).  n_atoms must be a multiple of group.
 */
typedef struct MdgCoulombConsts {
    double alpha, rc, c0, c1, g0, alpha2, conversion, self_s;
} MdgCoulombConsts;
int64_t mdg_coulomb_partial_size(int n_atoms);
int mdg_coulomb_eval(const float* pos, int n_atoms, const MdgCell* cell /*host*/, const int32_t* col, const int32_t* shift,
                     const int32_t* cnt, int max_nbr, const float* q, const MdgCoulombConsts* consts /*host*/, const float* w,
                     float* energy, float* grad, float* hw, float* pot, float* potw, float* partial, float out_scale,
                     int accumulate, void* stream);
int mdg_coulomb_charge_reduce(const float* val, const int32_t* types, int n_atoms, int group, int n_slots, float* out,
                              void* stream);

/* ------------------------------------------------------------------------------------
 * K21  reciprocal-space part of the Ewald sum for point charges (mdgrad_amd/interface.py EwaldReciprocal, csrc/ewald.hip).
 *      For one replica on a diagonal cell L = (Lx, Ly, Lz), V = Lx Ly Lz, with charges q_i and the wave vectors
 *      k(n) = 2 pi (nx / Lx, ny / Ly, nz / Lz), integer n != 0 of one half space (k and -k contribute equally), |k| <= k_cutoff:
 *        rho(k) = A + iB = sum_j q_j exp(i k.x_j)
 *        c(k)   = (4 pi / V) exp(-k^2 / (4 alpha^2)) / k^2                      (host, double -> the float table `coef`)
 *        U_rec  = conversion [ sum_k c(k) |rho(k)|^2  -  pi (sum_j q_j)^2 / (2 V alpha^2) ]
 *      The second term (the neutralising background; zero for a neutral cell), the conversion and the self term
 *      -alpha / sqrt(pi) sum q_i^2 (K20's self_s with shift "none") are the caller's: the kernels work on `coef` as given.
 *      With c_i = cos k.x_i, s_i = sin k.x_i, a direction w, kw_i = k.w_i and sigma(k) = sum_j q_j kw_j exp(i k.x_j):
 *        energy  = sum over replicas and k of coef(k) (A^2 + B^2)
 *        dU/dx_i = sum_k 2 coef q_i k (B c_i - A s_i)
 *        pot_i   = sum_k 2 coef (A c_i + B s_i)                                 (dU/dq_i before background and conversion)
 *        (H w)_i = sum_k 2 coef q_i k [ Re sigma c_i + Im sigma s_i - kw_i (A c_i + B s_i) ]
 *        potw_i  = sum_k 2 coef [ kw_i (B c_i - A s_i) + Re sigma s_i - Im sigma c_i ]       (d(w.dU/dx)/dq_i)
 *   mdg_ewald_eval  pos [n_rep, n_atoms, 3] (the replicas of System.replicate; positions need not be wrapped), q [n_rep,
 *     n_atoms], kvec int32 [n_vecs, 3] with |n_d| <= 1024 (the caller's guarantee: the table lives on the device), coef
 *     [n_vecs], w nullable [n_rep, n_atoms, 3] (required for hw / potw).  Limits: n_atoms <= 32 768, 1 <= n_vecs <= 65 536.
 *     workspace: mdg_ewald_workspace() floats; it holds (A, B, Re sigma, Im sigma) per (replica, vector) afterwards.
 *     Outputs, each nullable: energy [1]; grad [n_rep n_atoms, 3] = (accumulate & 1 ? grad : 0) + out_scale dU/dx, hw
 *     likewise with H w; pot, potw [n_rep n_atoms].  Three launches at most (modes, atoms, energy in double); every sum in
 *     a fixed order, no atomics: bitwise reproducible.
 */
int64_t mdg_ewald_workspace(int n_rep, int n_atoms, int n_vecs);
int mdg_ewald_eval(const float* pos, int n_rep, int n_atoms, const MdgCell* cell /*host*/, const float* q, const int32_t* kvec,
                   const float* coef, int n_vecs, const float* w, float* energy, float* grad, float* hw, float* pot, float* potw,
                   float* workspace, float out_scale, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K22  erf correction of the Ewald sum for excluded and scaled pairs (mdgrad_amd/interface.py EwaldExclusions,
 *      csrc/ewald_excl.hip).  The reciprocal sum K21 runs over all charges; for a static list of pairs p = (i, j) of one replica,
 *      each with a scale s_p in [0, 1], this term adds, with E1 = erf(alpha r), G = (2 alpha / sqrt(pi)) exp(-alpha^2 r^2):
 *        chi(r)   = (s - E1) / r
 *        chi'(r)  = -(s - E1) / r^2 - G / r
 *        chi''(r) = 2 (s - E1) / r^3 + 2 G / r^2 + 2 alpha^2 G
 *        U        = conversion * sum over the pairs of every replica of q_i q_j chi_{s_p}(r_ij)
 *      r_ij = |x_lo - x_hi| (lo = min(i, j)) re-imaged like a bond vector (topology.get_offsets on the diagonal cell:
 *      -[b >= L/2] + [b < -L/2], piecewise constant).  s = 0: the pair is excluded (K20's mask removes erfc/r, this removes the
 *      erf/r of K21); s = 1: chi is K20's psi with shift "none".  No self term, no background term.  Below alpha r = 1 the erf
 *      part comes from the power series of erf(x)/x (14 terms) -- the closed forms cancel in float32 -- and a coincident pair
 *      (r == 0) contributes its limits: energy -q_i q_j 2 alpha / sqrt(pi), zero gradient, (H w)_i = q_i q_j (4 alpha^3 /
 *      (3 sqrt(pi))) (w_i - w_j), pot -q_j 2 alpha / sqrt(pi), potw 0; the s / r part of such a pair is dropped.
 *   mdg_ewald_excl_eval  pos [n_rep, n_atoms, 3] (need not be wrapped), q [n_rep, n_atoms], cell_len host float[3];
 *     row_ptr int32 [n_atoms + 1], col int32 [nnz], scale float [nnz]: the CSR incidence list of one replica -- row(a) holds the
 *     partners of atom a in ascending order (every pair twice, once per end) with the pair's scale; all replicas share it.
 *     The caller guarantees 0 <= col < n_atoms and col != the row's atom.  w nullable [n_rep, n_atoms, 3] (required for hw /
 *     potw).  Outputs, each nullable: energy [1] (needs `partial`: mdg_ewald_excl_partial_size() doubles; per-block sums in
 *     double, then one fixed tree); grad [n_rep n_atoms, 3] = (accumulate & 1 ? grad : 0) + out_scale dU/dx, hw likewise with
 *     H w -- an atom with an empty row leaves an accumulated buffer untouched; pot_i = sum_j q_j chi(r_ij), potw_i = sum_j q_j
 *     chi'(r_ij) rhat_ij.(w_i - w_j) [n_rep n_atoms] (dU/dq_i = conversion pot_i).  One launch, plus the finish for the
 *     energy; every sum in a fixed order, no atomics: bitwise reproducible.
 */
int64_t mdg_ewald_excl_partial_size(int n_rep, int n_atoms);
int mdg_ewald_excl_eval(const float* pos, int n_rep, int n_atoms, const float* cell_len /*host*/, const int32_t* row_ptr,
                        const int32_t* col, const float* scale, const float* q, double alpha, double conversion, const float* w,
                        float* energy, float* grad, float* hw, float* pot, float* potw, double* partial, float out_scale,
                        int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K23  Stillinger-Weber two- plus three-body potential for one species over the per-atom (ELL) list (Stillinger and Weber
 *      1985; mW water: Molinero and Moore 2009; mdgrad_amd/interface.py StillingerWeber, csrc/sw.hip).  With rc = a sigma and
 *      g(r) = exp(gamma sigma / (r - rc)) for r < rc, exactly 0 otherwise:
 *        phi2(r)       = A eps [B (sigma/r)^p - (sigma/r)^q] exp(sigma / (r - rc))
 *        phi3(j, i, k) = lam eps (cos theta_jik - cos0)^2 g(r_ij) g(r_ik)                        (i = the centre)
 *        U = 1/2 sum_i sum_{j in row(i)} phi2(r_ij) + sum_i sum_{j < k in row(i)} phi3(j, i, k)
 *      The list may have been searched with any radius >= rc: every entry with r >= rc is skipped (r - rc is formed from
 *      r = sqrt(d2); the exponentials are expf).  Rows are not staged, so their length is not capped.
 *      MdgSWConsts holds the fixed constants and host copies of (epsilon, sigma, lam); `theta`, when not null, is a device
 *      float[3] = (epsilon, sigma, lam) that the kernel reads instead (trainable parameters under HIP-graph replay: no host
 *      value is baked into the launch).  Without theta the host values must satisfy epsilon > 0, sigma > 0, lam >= 0.
 *   mdg_sw_eval  laid out like mdg_coulomb_eval (same list, same `accumulate` bits: 1 = add onto grad / hw, 2 = the list was
 *     searched with a skin -- accepted, and nothing more to do: the support test is always applied; same out_scale).
 *     w nullable [n_atoms, 3], required for hw / pthw.  Outputs, each nullable:
 *       energy [1] = U (needs `partial`, mdg_sw_partial_size() floats; fixed-order block partials + a finish kernel)
 *       grad [n_atoms, 3] = (accumulate & 1 ? grad : 0) + out_scale dU/dx,  hw likewise with H w.  dU/dx_i gathers the pairs of
 *         i, the triplets centred on i, and the triplets centred on each neighbour j in which i is an end atom (the entries of
 *         row(j) with j's own stored images)
 *       pth [n_atoms, 3]  = d u_i / d(epsilon, sigma, lam) of u_i = 1/2 sum_j phi2 + the triplets centred on i
 *                           (their sums over i are dU/d(epsilon, sigma, lam))
 *       pthw [n_atoms, 3] = (w . grad_x) of the same three (their sums are d(w.dU/dx)/d(epsilon, sigma, lam))
 *     H w and pthw come from one pass over Dual numbers seeded with w (csrc/dual.hpp).  No atomics: bitwise reproducible; the
 *     value parts of a launch with w equal those of a launch without, bit for bit.
 */
typedef struct MdgSWConsts {
    double epsilon, sigma, lam, a, gamma, cos0, A, B;
    int32_t p, q;
} MdgSWConsts;
int64_t mdg_sw_partial_size(int n_atoms);
int mdg_sw_eval(const float* pos, int n_atoms, const MdgCell* cell /*host*/, const int32_t* col, const int32_t* shift,
                const int32_t* cnt, int max_nbr, const MdgSWConsts* consts /*host*/, const float* theta, const float* w,
                float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial, float out_scale,
                int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K24  Sutton-Chen (Finnis-Sinclair) embedded-atom potential for one species over the per-atom (ELL) list (Sutton and Chen
 *      1990; mdgrad_amd/interface.py SuttonChen, csrc/eam.hip).  With S_k(r) = (a/r)^k - (a/rc)^k + k (r - rc) (a/rc)^k / rc
 *      (shift = 1) or S_k(r) = (a/r)^k (shift = 0) for r < rc, exactly 0 otherwise:
 *        rho_i = sum_{j in row(i)} S_m(r_ij),   u_i = 1/2 epsilon sum_{j in row(i)} S_n(r_ij) - epsilon c sqrt(rho_i),   U = sum_i u_i
 *      An atom with rho_i = 0 (no neighbour inside rc) has embedding energy, F'(rho_i) and F''(rho_i) exactly 0.
 *      The list may have been searched with any radius >= rc: every entry with r = sqrt(d2) >= rc is skipped.  Rows are not
 *      staged, so their length is not capped.
 *      MdgEAMConsts holds the constants (rc, n, m, shift) and host copies of (epsilon, a, c); `theta`, when not null, is a
 *      device float[3] = (epsilon, a, c) that the kernels read instead (trainable parameters under HIP-graph replay).  Without
 *      theta the host values must satisfy epsilon > 0, a > 0, c >= 0.  Always: rc > 0, 1 <= m < n <= 16.
 *   mdg_eam_eval  argument for argument mdg_sw_eval (same list, same `accumulate` bits, same out_scale, same outputs) plus
 *     atom_work [n_atoms, 4], a caller-owned device scratch that must not be null: one call enqueues the density pass, which
 *     writes (rho_i, d rho_i, F'(rho_i), F''(rho_i) d rho_i) there (d rho_i = sum_j S_m'(r_ij) e_ij.(w_j - w_i), 0 without w),
 *     then the force pass, which reads the neighbours' entries, then the finish kernel of the energy.  Outputs, each nullable:
 *       energy [1] = U (needs `partial`, mdg_eam_partial_size() floats; fixed-order block partials + a finish kernel)
 *       grad [n_atoms, 3] = (accumulate & 1 ? grad : 0) + out_scale dU/dx,  hw likewise with H w, where
 *         dU/dx_i = -sum_j [epsilon S_n'(r_ij) + (F'_i + F'_j) S_m'(r_ij)] e_ij,  e_ij the unit vector i -> j
 *       pth [n_atoms, 3]  = (u_i / epsilon,  (n/2 epsilon sum_j S_n + m rho_i F'(rho_i)) / a,  -epsilon sqrt(rho_i))
 *                           = d u_i / d(epsilon, a, c)   (S_k is homogeneous of degree k in a; their sums over i are dU/dtheta)
 *       pthw [n_atoms, 3] = (w . grad_x) of the same three (their sums are d(w.dU/dx)/d(epsilon, a, c))
 *     H w and pthw come from both passes run over Dual numbers seeded with w (csrc/dual.hpp).  No atomics: bitwise
 *     reproducible; the value parts of a launch with w equal those of a launch without, bit for bit.
 */
typedef struct MdgEAMConsts {
    double epsilon, a, c, rc;
    int32_t n, m, shift, pad_;
} MdgEAMConsts;
int64_t mdg_eam_partial_size(int n_atoms);
int mdg_eam_eval(const float* pos, int n_atoms, const MdgCell* cell /*host*/, const int32_t* col, const int32_t* shift,
                 const int32_t* cnt, int max_nbr, const MdgEAMConsts* consts /*host*/, const float* theta, const float* w,
                 float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial, float* atom_work,
                 float out_scale, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K25  Tersoff bond-order potential for one species over the per-atom (ELL) list (Tersoff 1988, 1989; the LAMMPS convention;
 *      mdgrad_amd/interface.py Tersoff, csrc/tersoff.hip):
 *        U       = 1/2 sum_i sum_{j in row(i)} fc(r_ij) [A exp(-lam1 r_ij) - b_ij B exp(-lam2 r_ij)]
 *        b_ij    = (1 + (beta zeta_ij)^n)^(-1/(2n))
 *        zeta_ij = sum_{k in row(i), k != j} fc(r_ik) g(cos theta_jik) exp[(lam3 (r_ij - r_ik))^m]
 *        g(x)    = gamma (1 + c^2/d^2 - c^2/(d^2 + (h - x)^2)),  evaluated as gamma (1 + (c/d)^2 u^2 / (d^2 + u^2)), u = h - x
 *        fc(r)   = 1 for r <= R - D,  1/2 - 1/2 sin(pi (r - R) / (2 D)) for R - D < r < R + D,  exactly 0 for r >= R + D
 *      A bond with zeta_ij = 0 has b_ij = 1 and every derivative of b_ij exactly 0.
 *      The list may have been searched with any radius >= R + D: every entry with r = sqrt(d2) >= R + D is skipped.  Rows are
 *      not staged, so their length is not capped.
 *      MdgTersoffConsts holds the constants and host copies of (A, B, h); `theta`, when not null, is a device float[3] =
 *      (A, B, h) that the kernels read instead (trainable parameters under HIP-graph replay).  Without theta the host values
 *      must satisfy A > 0, B > 0.  Always: lam1 > 0, lam2 > 0, D > 0, R > D, m = 1 or 3, n > 0, beta >= 0, d != 0.
 *   mdg_tersoff_eval  argument for argument mdg_sw_eval (same list, same `accumulate` bits, same out_scale, same outputs) plus
 *     bond_work, a caller-owned device scratch of mdg_tersoff_work_size(n_atoms, max_nbr) floats (4 per list slot), required
 *     whenever grad or hw is requested: one call enqueues the bond pass, which writes (P, dP, b, db) of the bond in every slot
 *     (P = dU/dzeta; dP, db = their directional derivatives along w, 0 without w), then, for grad / hw, the force pass, which
 *     reads the entries of the atom's row and of its neighbours' rows, then the finish kernel of the energy.  Outputs, each
 *     nullable:
 *       energy [1] = U (needs `partial`, mdg_tersoff_partial_size() floats; fixed-order block partials + a finish kernel)
 *       grad [n_atoms, 3] = (accumulate & 1 ? grad : 0) + out_scale dU/dx,  hw likewise with H w
 *       pth [n_atoms, 3]  = d u_i / d(A, B, h) of u_i = 1/2 sum_{j in row(i)} fc (A exp(-lam1 r) - b_ij B exp(-lam2 r))
 *                           (their sums over i are dU/d(A, B, h))
 *       pthw [n_atoms, 3] = (w . grad_x) of the same three (their sums are d(w.dU/dx)/d(A, B, h))
 *     H w and pthw come from both passes run over Dual numbers seeded with w (csrc/dual.hpp).  No atomics: bitwise
 *     reproducible; the value parts of a launch with w equal those of a launch without, bit for bit.
 */
typedef struct MdgTersoffConsts {
    double A, B, lam1, lam2, beta, n, c, d, h, R, D, lam3, gamma;
    int32_t m, pad_;
} MdgTersoffConsts;
int64_t mdg_tersoff_partial_size(int n_atoms);
int64_t mdg_tersoff_work_size(int n_atoms, int max_nbr);
int mdg_tersoff_eval(const float* pos, int n_atoms, const MdgCell* cell /*host*/, const int32_t* col, const int32_t* shift,
                     const int32_t* cnt, int max_nbr, const MdgTersoffConsts* consts /*host*/, const float* theta,
                     const float* w, float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial,
                     float* bond_work, float out_scale, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K26  Tersoff bond-order potential for 1 <= S <= 4 species over the per-atom (ELL) list (Tersoff 1989, the multicomponent
 *      paper; the LAMMPS convention with lam3 = 0; mdgrad_amd/interface.py TersoffMulti, csrc/tersoff_multi.hip).  With
 *      a = types[i], b = types[j], c = types[k]:
 *        U       = 1/2 sum_i sum_{j in row(i)} fc_ab(r_ij) [A_ab exp(-lam1_ab r_ij) - b_ij B_ab exp(-lam2_ab r_ij)]
 *        b_ij    = (1 + (beta_a zeta_ij)^n_a)^(-1/(2 n_a)),   exactly 1 with zero derivatives where zeta_ij = 0
 *        zeta_ij = sum_{k in row(i), k != j} fc_ac(r_ik) g_a(cos theta_jik)
 *        g_a(x)  = gamma_a (1 + c_a^2/d_a^2 - c_a^2/(d_a^2 + (h_a - x)^2))
 *        fc_ab   = 1 for r <= R_ab - D_ab,  1/2 - 1/2 sin(pi (r - R_ab) / (2 D_ab)) inside,  exactly 0 for r >= R_ab + D_ab
 *      `types`: device int32 [n_atoms], values in [0, S) (checked by the caller; the kernels clamp what they read).
 *      `tables`: device float [mdg_tersoff_multi_table_size(S)] = 8 S (S + 1) derived constants,
 *        pair entry   tables[8 (a S + b) ...] = A, B, lam1, lam2, R, R - D, R + D, pi / (2 D)      (row = centre, column = end;
 *                                               (a, b) and (b, a) are separate entries and may differ)
 *        centre entry tables[8 S S + 8 a ...] = h, beta, n, -1/(2n), d^2, gamma, gamma (c/d)^2, 2 gamma (c/d)^2 d^2
 *      The caller validates the entries (mdgrad_amd/ops.py tersoff_multi_tables: A, B, lam1, lam2 > 0, D > 0, R > D, n > 0,
 *      beta >= 0, d != 0); being device data they are not read here.  The list may have been searched with any radius >=
 *      max_ab (R_ab + D_ab): every entry is tested against the support of its own pair entry.
 *   mdg_tersoff_multi_eval  the passes, bond_work, `accumulate`, out_scale and the outputs energy, grad, hw of
 *     mdg_tersoff_eval (K25); mdg_tersoff_multi_work_size(n_atoms, max_nbr) floats of bond_work, required for grad or hw;
 *     mdg_tersoff_multi_partial_size(n_atoms) floats of `partial`, required for energy.  The per-atom parameter outputs are
 *       pth [n_atoms, 2 S S + S]  row i = d u_i / d(A [S, S], B [S, S], h [S]), flattened in that order: u_i depends on
 *                                 A[a, :], B[a, :], h[a] only, every other word of the row is written as 0, so the column
 *                                 sums over the atoms (one GRAD_COLSUM job of mdg_grad_jobs) are dU/d(A, B, h)
 *       pthw, the same shape      (w . grad_x) of the same (the column sums are d(w.dU/dx)/d(A, B, h))
 *     n_species outside [1, 4], null types or tables, grad / hw without bond_work: MDG_EINVAL.  No atomics: bitwise
 *     reproducible; the value parts of a launch with w equal those of a launch without, bit for bit.
 */
int64_t mdg_tersoff_multi_partial_size(int n_atoms);
int64_t mdg_tersoff_multi_work_size(int n_atoms, int max_nbr);
int64_t mdg_tersoff_multi_table_size(int n_species);
int mdg_tersoff_multi_eval(const float* pos, int n_atoms, const MdgCell* cell /*host*/, const int32_t* col, const int32_t* shift,
                           const int32_t* cnt, int max_nbr, const int32_t* types, int n_species, const float* tables /*device*/,
                           const float* w, float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial,
                           float* bond_work, float out_scale, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K27  Tabulated embedded-atom potential ("eam/alloy") for 1 <= S <= 4 species over the per-atom (ELL) list
 *      (mdgrad_amd/interface.py EAM, csrc/eam_table.hip).  With a = types[i], b = types[j]:
 *        rho_i = sum_{j in row(i)} f_b(r_ij),   u_i = 1/2 sum_{j in row(i)} phi_ab(r_ij) + F_a(rho_i),   U = sum_i u_i
 *      Every function is a cubic-Hermite interpolant on a uniform grid with node entries (value, h * derivative), the
 *      convention of MDG_PAIR_TABLE.  phi and f live on r_g = r_min + g h_r, g = 0 .. n_r - 1, with r_{n_r - 1} = rc; F on
 *      rho_g = rho_min + g h_rho, g = 0 .. n_rho - 1.  Outside its grid (r < r_min; rho < rho_min or rho > rho_max) a function
 *      continues linearly with the end node's value and slope.  An atom with an empty row has rho_i = 0 and gets F_a(0) from
 *      the table (not the "exactly 0" rule of K24).  Every entry with r = sqrt(d2) >= rc or r = 0 is skipped, so the list may
 *      have been searched with any radius >= rc.
 *      `types`: device int32 [n_atoms], values in [0, S) (checked by the caller; the kernels clamp what they read).
 *      `tables`: device float [mdg_eam_table_size(S, n_r, n_rho)], the node entries in the order
 *        pair [S (S + 1) / 2, n_r, 2]   phi of the unordered pair (a, b) at index hi (hi + 1) / 2 + lo  (the lower triangle)
 *        density [S, n_r, 2]            f_b: the density an atom of species b contributes
 *        embed [S, n_rho, 2]            F_a
 *      Being device data they are not read here.  MdgEAMTableConsts holds the grids: n_species, n_r, n_rho, r_min, h_r, rc,
 *      rho_min, h_rho, and pin_cutoff (1: the gradient of the last node of every phi and f table is returned as exactly 0).
 *   mdg_eam_table_eval  the passes, atom_work [n_atoms, 4], `accumulate`, out_scale and the outputs energy, grad, hw of
 *     mdg_eam_eval (K24), with  dU/dx_i = -sum_j [phi_ab'(r_ij) + F_a'(rho_i) f_b'(r_ij) + F_b'(rho_j) f_a'(r_ij)] e_ij;
 *     mdg_eam_table_partial_size(n_atoms) floats of `partial`, required for energy.  The parameter outputs are
 *       gtab [mdg_eam_table_size()]   dU/dtables, the layout of `tables` (a call without w)
 *       gtabw, the same shape         d(w.dU/dx)/dtables (a call with w)
 *     Either needs `fx`, a caller-owned device scratch of mdg_eam_table_fx_size(S, n_r, n_rho) int64 words: the contributions
 *     (1/2 basis(r_ij) to phi_ab and F_a'(rho_i) basis(r_ij) to f_b per list entry, basis(rho_i) to F_a per atom; with w their
 *     directional derivatives) are added as fixed-point numbers with integer atomics, one word per entry, at a power-of-two
 *     scale per table family that the density pass derives on the device from measured upper bounds (max |basis|, max |F'|,
 *     max |F'' d rho|) so that no sum can leave 2^62: order-independent, no flag, no host read.  A table set of at most 6144
 *     words is summed per workgroup in LDS first (48 KiB at most), a larger one in global memory alone.  A finish kernel
 *     writes the floats.  MDG_EINVAL: a null buffer, n_species outside [1, 4], n_r or n_rho outside [4, 4096], h_r <= 0 or h_rho <= 0,
 *     rc <= r_min, r_min < 0, hw / gtabw without w, w without hw or gtabw, gtab together with w, gtab / gtabw without fx.
 *     No float atomics: bitwise reproducible; the value parts of a launch with w equal those of a launch without, bit for bit.
 *   mdg_eam_table_size / _fx_size return -1 for sizes outside the limits.
 */
typedef struct MdgEAMTableConsts {
    double r_min, h_r, rc, rho_min, h_rho;
    int32_t n_species, n_r, n_rho, pin_cutoff;
} MdgEAMTableConsts;
int64_t mdg_eam_table_partial_size(int n_atoms);
int64_t mdg_eam_table_size(int n_species, int n_r, int n_rho);
int64_t mdg_eam_table_fx_size(int n_species, int n_r, int n_rho);
int mdg_eam_table_eval(const float* pos, int n_atoms, const MdgCell* cell /*host*/, const int32_t* col, const int32_t* shift,
                       const int32_t* cnt, int max_nbr, const int32_t* types, const MdgEAMTableConsts* consts /*host*/,
                       const float* tables /*device*/, const float* w, float* energy, float* grad, float* hw, float* gtab,
                       float* gtabw, float* partial, float* atom_work, int64_t* fx, float out_scale, int accumulate,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * K28  Stillinger-Weber potential for 1 <= S <= 4 species over the per-atom (ELL) list (the LAMMPS `pair_style sw`
 *      convention; mdgrad_amd/interface.py StillingerWeberMulti, csrc/sw_multi.hip).  With a = types[i] (the centre),
 *      b = types[j], c = types[k]:
 *        U        = 1/2 sum_i sum_{j in row(i)} phi2_ab(r_ij) + sum_i sum_{j<k in row(i)} phi3_abc(r_ij, r_ik, cos theta_jik)
 *        phi2_ab  = A_ab eps_ab [B_ab (sigma_ab/r)^p_ab - (sigma_ab/r)^q_ab] exp(sigma_ab / (r - a_ab sigma_ab))
 *        g_ab     = exp(gamma_ab sigma_ab / (r - a_ab sigma_ab)),      both exactly 0 for r >= a_ab sigma_ab
 *        phi3_abc = K_a{bc} (cos theta - cos0_abc)^2 g_ab(r_ij) g_ac(r_ik),   K_a{bc} = (lam_abc eps3_abc + lam_acb eps3_acb) / 2
 *      `types`: device int32 [n_atoms], values in [0, S) (checked by the caller; the kernel clamps what it reads).
 *      `tables`: device float [mdg_sw_multi_table_size(S)] = 12 S S + 4 S S S derived constants,
 *        pair entry    tables[12 (a S + b) ...]                 = eps, sigma, a sigma, gamma sigma, gamma, A, B, p, q, a, A eps, 0
 *                                                                 (row = centre, column = end; (a, b) and (b, a) are separate
 *                                                                 entries and may differ; p, q integers, 0 <= q < p <= 12)
 *        triplet entry tables[12 S S + 4 ((a S + b) S + c) ...] = K_a{bc}, cos0_abc, w_abc, 0
 *                                                                 (K and cos0 symmetric in b, c; w_abc = eps3_abc / 2, eps3_abb
 *                                                                 for b = c: d K_a{bc} / d lam_abc)
 *      The caller validates the entries (mdgrad_amd/ops.py sw_multi_tables); being device data they are not read here.  The
 *      list may have been searched with any radius >= max_ab a_ab sigma_ab: every entry is tested against the support of its
 *      own pair entry.  With asymmetric pair tables the force of a pair is the derivative of (phi2_ab + phi2_ba) / 2.
 *   mdg_sw_multi_eval  one launch, laid out like mdg_sw_eval (K23): the same list, `accumulate` bits, out_scale and the outputs
 *     energy, grad, hw; mdg_sw_multi_partial_size(n_atoms) floats of `partial`, required for energy.  The per-atom parameter
 *     outputs are
 *       pth [n_atoms, 2 S S + S S S]  row i = d u_i / d(eps [S, S], sigma [S, S], lam [S, S, S]), flattened in that order, of
 *                                     u_i = 1/2 sum_j phi2_ab + the triplets centred on i: it depends on eps[a, :],
 *                                     sigma[a, :], lam[a, :, :] only, every other word of the row is written as 0, and
 *                                     lam[a, b, c], lam[a, c, b] hold w_abc, w_acb times the sum of their unordered class, so
 *                                     the column sums over the atoms (one GRAD_COLSUM job of mdg_grad_jobs) are
 *                                     dU/d(eps, sigma, lam)
 *       pthw, the same shape          (w . grad_x) of the same (the column sums are d(w.dU/dx)/d(eps, sigma, lam))
 *     n_species outside [1, 4], null types or tables: MDG_EINVAL.  No atomics: bitwise reproducible; the value parts of a
 *     launch with w equal those of a launch without, bit for bit.
 *   mdg_sw_multi_table_size returns 0 for n_species outside [1, 4].
 */
int64_t mdg_sw_multi_partial_size(int n_atoms);
int64_t mdg_sw_multi_table_size(int n_species);
int mdg_sw_multi_eval(const float* pos, int n_atoms, const MdgCell* cell /*host*/, const int32_t* col, const int32_t* shift,
                      const int32_t* cnt, int max_nbr, const int32_t* types, int n_species, const float* tables /*device*/,
                      const float* w, float* energy, float* grad, float* hw, float* pth, float* pthw, float* partial,
                      float out_scale, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K29  Steinhardt bond-orientational order: per-atom moments over the per-atom (ELL) list and their gradient
 *      (mdgrad_amd/observable.py bond_order; no counterpart in the reference; csrc/bond_order.hip)
 *   pos [n_frames * n_atoms, 3]; col / cnt: the ELL list of K1 over those rows (frames = groups of n_atoms, col holds row
 *   indices; it must be symmetric, as the builders make it); the cell must be diagonal.  For every row i and every entry j of
 *   its list row: u = x_j - x_i re-imaged like the list builder, r = |u|, s = u / r,
 *     w(r) = 1 (r <= r_in), 1/2 [1 + cos(pi (r - r_in) / (cutoff - r_in))] (r_in < r < cutoff), 0 (r >= cutoff);  0 < r_in < cutoff
 *     A_lm(i) = sum_j w(r_ij) Y_lm(s_ij),  n_i = sum_j w(r_ij),   Y_lm the real orthonormal spherical harmonics
 *   ls: HOST int32 [n_l], 1 <= n_l <= 4 distinct values in [1, 12]; K = sum (2l+1) = mdg_bond_order_components(ls, n_l)
 *   (0 for a refused ls).  Component k of an l's block of 2l+1: k = l - m the sine component of order m, k = l the m = 0 one,
 *   k = l + m the cosine one; the blocks follow the order of ls.
 *   fwd: A [K, n_frames * n_atoms] COMPONENT-MAJOR (a wave stores 256 contiguous bytes per component) and n [n_frames * n_atoms].
 *   bwd: given gA [n_frames * n_atoms, K] ROW-MAJOR (the gather of a neighbour's 2l+1 entries stays inside one or two cache
 *        lines) and gn [n_frames * n_atoms], the cotangents of A and n, writes g_xyz [n_frames * n_atoms, 3].
 *   One thread per row, one l at a time, fixed-order sums, no atomics, no workspace: bitwise reproducible.  A row whose own
 *   position is not finite gets NaN outputs; cnt is clamped to [0, max_nbr] and a column outside the row's frame is skipped.
 *   A refused ls or n_l is MDG_EINVAL before anything else is looked at.
 */
int mdg_bond_order_components(const int32_t* ls /*host*/, int n_l);
int mdg_bond_order_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff, float r_in,
                       const int32_t* col, const int32_t* cnt, int max_nbr, const int32_t* ls /*host*/, int n_l, float* A, float* n,
                       void* stream);
int mdg_bond_order_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff, float r_in,
                       const int32_t* col, const int32_t* cnt, int max_nbr, const int32_t* ls /*host*/, int n_l, const float* gA,
                       const float* gn, float* g_xyz, void* stream);

/* ------------------------------------------------------------------------------------
 * K31  pair potential energy of every frame and its gradient (mdgrad_amd/thermo.py PotentialEnergy; the energy side of
 *      trajectory reweighting, mdgrad_amd/reweight.py; csrc/energy.hip on the sweeps of csrc/frame_pairs.hpp)
 *   pos, cell, terms, theta, the pair set and the three kernel shapes: as K15.
 *   U[f] = sum_terms sum_pairs phi(r), the plain truncated phi (no shift): the value PairPotentials gives for frame f.
 *   fwd: U[n_frames], every unordered pair once.
 *   bwd: given gU[n_frames] = dL/dU.  g_pos and g_theta are each nullable (not both):
 *        g_pos != null   full rows: g_pos [n_frames, n_atoms, 3] = -gU_f sum_j phi'(r) (x_j - x_i) / r, and g_theta (when not
 *                        null) = sum_f gU_f sum_pairs dphi/dtheta from half of each visit
 *        g_pos == null   parameters only (the frames are constants, as in reweighting): the forward's once-per-pair sweep
 *                        accumulating g_theta[n_theta_total] alone -- half the pair visits, no position written
 *   workspace: mdg_energy_frames_workspace() floats, shared by both calls.  Fixed-order sums, no floating-point atomics:
 *   bitwise reproducible.  Tabulated terms (MDG_PAIR_TABLE) are refused: their energy is not tabulated.
 */
int64_t mdg_energy_frames_workspace(int n_frames, int n_atoms, int n_theta_total);
int mdg_energy_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/,
                          const float* theta, float* U, float* workspace, void* stream);
int mdg_energy_frames_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const MdgTerms* terms /*host*/,
                          const float* theta, const float* gU, float* g_pos, float* g_theta, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * K32  smeared pair count of every frame and its gradient (mdgrad_amd/observable.py rdf.per_frame; csrc/rdf_frames.hip):
 *      the rows whose sum over frames K4 returns
 *   pos [n_frames, n_atoms, 3], n_atoms <= 1024; the cell must be diagonal; mask: nullable [n_atoms, n_atoms] uint8 selection
 *   (symmetric); mu [nbins] DEVICE: equally spaced ascending centres, spacing = mu[1] - mu[0] > 0; coeff < 0; 2 <= nbins <= 1024.
 *     raw[f, k] = sum_{i<j, 0 < d^2 < cutoff^2} exp(coeff (d - mu_k)^2)
 *   over the 2R + 1 centres around the nearest one, R = ceil(5.3 / (s spacing)), s = sqrt(-coeff log2 e): a dropped term is
 *   <= 2^-28.1 of a peak term.
 *   fwd: raw [n_frames, nbins].  A frame belongs to one wave (n_atoms <= 128) or workgroup; its contributions are summed as
 *        fixed-point integers in LDS: bitwise reproducible, no global atomics.
 *   bwd: given g_raw [n_frames, nbins], writes g_xyz [n_frames, n_atoms, 3] = d(sum_fk g_raw raw)/d pos; atom-centric full
 *        rows, no atomics.  A frame whose g_raw row is zero gets zeros.
 */
int mdg_rdf_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff, const uint8_t* mask,
                       const float* mu, float spacing, float coeff, int nbins, float* raw, void* stream);
int mdg_rdf_frames_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, float cutoff, const uint8_t* mask,
                       const float* mu, float spacing, float coeff, int nbins, const float* g_raw, float* g_xyz, void* stream);

/* ------------------------------------------------------------------------------------
 * K33  tabulated pair energy of every frame and its gradient (mdgrad_amd/thermo.py TabulatedEnergy: reweighting of learned pair
 *      potentials, whose energy K31 refuses; csrc/energy_table.hip)
 *   pos, cell, mask, the pair set and the three kernel shapes: as K31, for ONE cutoff and ONE nullable mask.
 *   table [2 n_nodes] DEVICE: the nodes (phi_g, du * dphi/du_g) of phi on the grid u_g = u0 + g du in u = r^2, g = 0 .. n_nodes - 1,
 *   4 <= n_nodes <= 4096, du > 0, u0 >= 0, and the last node at cutoff^2 (to rounding): the layout and cubic-Hermite
 *   convention of MDG_PAIR_TABLE, applied to the energy.
 *     U[f] = sum_{i<j, 0 < d^2 < cutoff^2} phi~(d^2),  phi~ the interpolant; a pair with d^2 < u0 takes the constant first
 *     node value: no position gradient, its node gradient into entry 0.
 *   fwd: U[n_frames], every unordered pair once; n_below (one DEVICE int32) = the number of pairs with d^2 < u0.
 *   bwd: given gU[n_frames] = dL/dU.  g_pos and g_table are each nullable (not both):
 *        g_pos != null   full rows: g_pos [n_frames, n_atoms, 3] = -gU_f sum_j 2 (dphi~/du) (x_j - x_i), the exact derivative
 *                        of the interpolant, and g_table (when not null) from half of each visit
 *        g_pos == null   nodes only (the frames are constants, as in reweighting): the forward's once-per-pair sweep
 *                        accumulating g_table [2 n_nodes] = sum_f gU_f sum_pairs basis alone
 *   g_table is summed in fixed point with integer atomics (the scale is taken on the device from max |gU|: no host read) and
 *   U in a fixed order: bitwise reproducible, no floating-point atomics; both routes give the same g_table bits.
 *   workspace: mdg_energy_table_workspace() floats, shared by both calls.
 */
int64_t mdg_energy_table_workspace(int n_frames, int n_atoms, int n_nodes);
int mdg_energy_table_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const float* table, int n_nodes,
                         float u0, float du, float cutoff, const uint8_t* mask, float* U, int32_t* n_below, float* workspace,
                         void* stream);
int mdg_energy_table_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const float* table, int n_nodes,
                         float u0, float du, float cutoff, const uint8_t* mask, const float* gU, float* g_pos, float* g_table,
                         float* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * K34  Stillinger-Weber energy of every frame, list-free (mdgrad_amd/thermo.py StillingerWeberEnergy: reweighting of the
 *      one-species three-body model of K23; csrc/sw_frames.hip)
 *   pos [n_frames, n_atoms, 3], n_atoms <= 1024; the cell must be diagonal; consts: the fixed constants of MdgSWConsts (its host
 *   copies of epsilon, sigma, lam are not read); theta: DEVICE float[3] = (epsilon, sigma, lam), required.
 *     U[f] = 1/2 sum_i sum_j phi2(r_ij) + sum_i sum_{j<k} phi3(j, i, k)          K23's definition and per-edge formulas
 *   over the atoms j, k of frame f with D = x_j - x_i re-imaged by the strict minimum image (as K31) and 0 < r < a sigma,
 *   r = sqrtf(d2), with the live device sigma: U[f] is the value StillingerWeber gives for frame f.  No list and no host read:
 *   every atom finds its neighbours in the frame staged in LDS and keeps their indices in a compact row there.
 *   dU_dtheta nullable [n_frames, 3] = dU[f]/d(epsilon, sigma, lam) from the same pass; the value part of U does not depend on
 *   whether it is asked for, bit for bit.
 *   Row cap: mdg_sw_frames_row_cap() = 64 neighbours inside a sigma (silicon, mW water: 4 - 30).  A frame in which an atom
 *   has more comes out NaN (U and dU_dtheta), alone: rows are never truncated.
 *   Fixed-order sums, no floating-point atomics: bitwise reproducible, and permuting the frames permutes the outputs bit for
 *   bit.  Needs no workspace.
 *   mdg_sw_frames_theta_bwd: g_theta[3] = sum_f gU[f] dU_dtheta[f, :] in a fixed order -- the whole parameter backward pass of
 *   K34 (no second walk over the frames).  It is mdg_frames_theta_bwd (below) with n_params = 3: the same kernel
 *   (csrc/frames_reduce.hip), the same bits.
 */
int mdg_sw_frames_row_cap(void);
int mdg_sw_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const MdgSWConsts* consts /*host*/,
                      const float* theta, float* U, float* dU_dtheta, void* stream);
int mdg_sw_frames_theta_bwd(const float* gU, const float* dU_dtheta, int n_frames, float* g_theta, void* stream);

/* ------------------------------------------------------------------------------------
 * K36  tabulated embedded-atom energy of every frame, list-free (mdgrad_amd/thermo.py EAMEnergy: reweighting of the "eam/alloy"
 *      term of K27; csrc/eam_frames.hip)
 *   pos [n_frames, n_atoms, 3], n_atoms <= 1024, n_frames < 2^24; the cell must be diagonal; types: device int32 [n_atoms], the
 *   species of the atoms of ONE frame (values clamped into [0, S)); consts, tables: the grids and the flat node image of K27.
 *     U[f] = sum_i [ 1/2 sum_j phi_ab(r_ij) + F_a(rho_i) ],   rho_i = sum_j f_b(r_ij)          K27's definition and lookups
 *   over the atoms j of frame f with D = x_j - x_i re-imaged by the strict minimum image (as K31) and 0 < r < rc, r = sqrtf(d2):
 *   U[f] is the value the EAM term gives for frame f (linear continuation outside the grids; an atom without a neighbour gets
 *   F_a(0)).  Every atom walks its frame, staged in LDS, once: one bracketing cell per pair serves phi_ab and f_b, and F_a is
 *   applied when the walk ends.  No list, no row cap, no workspace.
 *   table_mode: where the pair and density tables are read from: 1 = a workgroup copy in LDS (at most
 *   mdg_eam_table_frames_lds_floats() floats of them, else MDG_EINVAL), 0 = global memory through the caches, -1 = the copy when
 *   the tables fit it and n_atoms <= 128 (four frames share it), global memory otherwise.
 *   The bits of U do not depend on it.
 *   rho nullable [n_frames, n_atoms] = rho_i of every atom, the input of the node gradient; the value part of U does not depend
 *   on whether it is asked for, bit for bit.
 *   mdg_eam_table_frames_nodes_bwd: g_tables [mdg_eam_table_size()] = sum_f gU[f] dU[f]/dtables in the layout of `tables`, from
 *   the frames, the saved rho and the tables: the forward walk once more, adding 1/2 gU_f basis(r_ij) to phi_ab and
 *   gU_f F_a'(rho_i) basis(r_ij) to f_b per visit, gU_f basis(rho_i) to F_a per atom, as fixed-point numbers with integer
 *   atomics (one int64 word per entry in `fx`, mdg_eam_table_fx_size() words; a table set of at most 6144 words is summed per
 *   workgroup in LDS first).  The power-of-two scale of each table family is taken on the device from bounds -- max |gU|,
 *   max |F'| and max |basis(rho)| over the saved rho, max(1, r_min / h_r) for basis(r), and n_frames n_atoms (n_atoms - 1)
 *   resp. n_frames n_atoms contributions -- so that no sum can leave 2^62: no flag, no host read (a captured graph can hold the
 *   call).  With pin_cutoff the last node of every phi and f table comes back as exactly 0.
 *   Fixed-order float sums and integer atomics only: bitwise reproducible; permuting the frames permutes U bit for bit and
 *   leaves g_tables unchanged bit for bit.  MDG_EINVAL: a null buffer, n_atoms > 1024, a non-diagonal cell, and the grid limits
 *   of K27 (n_species outside [1, 4], n_r or n_rho outside [4, 4096], h_r <= 0 or h_rho <= 0, rc <= r_min, r_min < 0).
 *
 * K37  Sutton-Chen energy of every frame, list-free (EAMEnergy for the one-species term of K24; csrc/eam_frames.hip)
 *   The skeleton of K36 with the closed-form S_n, S_m of K24 (csrc/eam_core.hpp); consts: rc, n, m, shift of MdgEAMConsts (its
 *   host copies of epsilon, a, c are not read); theta: DEVICE float[3] = (epsilon, a, c), required.  An atom without a neighbour
 *   has an embedding energy of exactly 0.
 *   dU_dtheta nullable [n_frames, 3] = dU[f]/d(epsilon, a, c) from the same pass (K24's pth formulas); the value part of U does
 *   not depend on whether it is asked for, bit for bit.  The parameter backward pass is mdg_frames_theta_bwd (below): the
 *   fixed-order weighted sum over the frames, no second walk.
 *   MDG_EINVAL: a null buffer, n_atoms > 1024, a non-diagonal cell, rc <= 0, exponents outside 1 <= m < n <= 16, shift not 0 / 1.
 */
int mdg_eam_table_frames_lds_floats(void);
int mdg_eam_table_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const int32_t* types,
                             const MdgEAMTableConsts* consts /*host*/, const float* tables /*device*/, int table_mode, float* U,
                             float* rho, void* stream);
int mdg_eam_table_frames_nodes_bwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const int32_t* types,
                                   const MdgEAMTableConsts* consts /*host*/, const float* tables /*device*/, const float* gU,
                                   const float* rho, float* g_tables, int64_t* fx, void* stream);
int mdg_eam_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/, const MdgEAMConsts* consts /*host*/,
                       const float* theta, float* U, float* dU_dtheta, void* stream);

/* ------------------------------------------------------------------------------------
 * K38  Tersoff energy of every frame, list-free (mdgrad_amd/thermo.py TersoffEnergy: reweighting of the bond-order models of
 *      K25 and K26; csrc/tersoff_frames.hip)
 *   pos [n_frames, n_atoms, 3], n_atoms <= 1024; the cell must be diagonal.
 *     U[f] = 1/2 sum_i sum_{j in row(i)} fc_ab(r_ij) [A_ab exp(-lam1_ab r_ij) - b_ij B_ab exp(-lam2_ab r_ij)]
 *   with K25 / K26's definition and formulas (csrc/tersoff_core.hpp) over the neighbours an atom finds in its own frame:
 *   D = x_j - x_i under the strict minimum image, 0 < r < R_ab + D_ab on r = sqrtf(d2) with the entry of the directed pair
 *   (centre species, end species); a bond with zeta = 0 has b = 1 and zero derivatives.  Only the bond pass runs: no list, no
 *   bond_work, no workspace.
 *   mdg_tersoff_frames_fwd        one species: consts = the constants of MdgTersoffConsts (its host copies of A, B, h are not
 *                                 read); theta: DEVICE float[3] = (A, B, h), required.  dU_dtheta nullable [n_frames, 3].
 *   mdg_tersoff_multi_frames_fwd  1 <= n_species <= 4: types DEVICE int32 [n_atoms] = one frame's species, shared by all frames
 *                                 (clamped into the table); tables: DEVICE float [mdg_tersoff_multi_table_size(n_species)], the
 *                                 image of K26.  dU_dtheta nullable [n_frames, 2 S^2 + S] in the order (A.flat, B.flat, h) of
 *                                 K26's pth.
 *   dU_dtheta comes from the same pass; the value part of U does not depend on whether it is asked for, bit for bit.
 *   Row cap: mdg_tersoff_frames_row_cap() = 32 neighbours inside R + D (silicon, carbon, germanium and their alloys: 3 - 10).
 *   A frame in which an atom has more comes out NaN (U and its dU_dtheta row), alone: rows are never truncated.
 *   Fixed-order sums, no floating-point atomics: bitwise reproducible, and permuting the frames permutes the outputs bit for
 *   bit.
 *   mdg_frames_theta_bwd: g_theta[n_params] = sum_f gU[f] dU_dtheta[f, :] in double and in a fixed order, a workgroup per
 *   parameter -- the whole parameter backward pass of K34, K37 and K38 (no second walk over the frames;
 *   csrc/frames_reduce.hip).
 *   MDG_EINVAL: a null buffer, n_atoms > 1024, a non-diagonal cell, n_species outside [1, 4], and for the one-species entry the
 *   conditions of mdg_tersoff_eval on the constants (lam1, lam2 > 0; D > 0; R > D; m = 1 or 3; n > 0; beta >= 0; d != 0).
 */
int mdg_tersoff_frames_row_cap(void);
int mdg_tersoff_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/,
                           const MdgTersoffConsts* consts /*host*/, const float* theta /*device [3], required*/, float* U,
                           float* dU_dtheta /*[F, 3] or null*/, void* stream);
int mdg_tersoff_multi_frames_fwd(const float* pos, int n_frames, int n_atoms, const MdgCell* cell /*host*/,
                                 const int32_t* types /*device [n_atoms]*/, int n_species, const float* tables /*device*/,
                                 float* U, float* dU_dtheta /*[F, 2 S^2 + S] or null*/, void* stream);
int mdg_frames_theta_bwd(const float* gU, const float* dU_dtheta, int n_frames, int n_params, float* g_theta, void* stream);

/* ------------------------------------------------------------------------------------
 * f4  bonded terms over a static topology table (csrc/bonded.hip).
 * Replaces torchmd/interface.py:447-455 (BondPotentials.forward: harmonic in the SQUARED bond length,
 * 1/2 k (|b|^2 - ro)^2) and :496-508 (AnglePotentials.forward: 1/2 k (theta - theta0)^2 over triples (i, j, k) centred on
 * j), their image flags topology.get_offsets (topology.py:75-80: -[b >= L/2] + [b < -L/2], L = cell.diag()), the autograd
 * force behind them (torchmd/md.py:228-230) and the double-backward Hessian-vector product of the adjoint
 * (torchmd/sovlers.py:229-233) -- one launch, no atomics.
 *   kind      MDG_BONDED_BOND: top = int32 [n_terms, 2], x0 = ro ;  MDG_BONDED_ANGLE: top = int32 [n_terms, 3], x0 = theta0
 *   cell_len  host float[3], the diagonal of the cell
 *   inc_ptr   int32 [n_atoms + 1], inc int32 [sum of roles]: the incidence list of every atom, entries 4 * term + role
 *             (role = the atom's column in `top`), ascending per atom -- the order the per-atom sums run in
 *   w         nullable [n_atoms, 3]; required for hw
 *   e_atom    nullable [n_atoms]: energy of the terms whose FIRST atom this is (sum = U)
 *   grad, hw  nullable [n_atoms, 3]:  grad = (accumulate ? grad : 0) + out_scale * dU/dx ,  hw likewise with H w
 *             (out_scale = -1: the force and d(w.F)/dx, added onto another Stack member's buffers when accumulate != 0)
 */
#define MDG_BONDED_BOND 0
#define MDG_BONDED_ANGLE 1
int mdg_bonded_eval(const float* pos, int n_atoms, const float* cell_len /*host*/, int kind, const int32_t* top, int n_terms,
                    float k, float x0, const int32_t* inc_ptr, const int32_t* inc, const float* w, float* e_atom,
                    float* grad, float* hw, float out_scale, int accumulate, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* MDGRAD_HIP_H */
