/*
 * hakai_hip.h -- C ABI of libhakai_hip.so: the MI355X (gfx950) explicit-dynamics inner loop of
 * HAKAI (yozoyugen/HAKAI-fem v0.0.2), behind HAKAI's own driver surface
 * (HAKAI("*.inp") -> temp/fileNNN.vtk).
 *
 * Reference files (read-only, /root/reference):  "v2/" = HAKAI-v0.0.2/Julia/
 *   v2/HAKAI_j.jl        solver; time loop :487-951
 *   v2/readInpFile_j.jl  .inp reader, :152-1113
 *
 * Conventions (identical to the reference's Julia arrays):
 *   - reals are FP64; index arrays are int64 and 1-BASED (elementmat, element_material, dofs);
 *   - coordmat/position are 3 x nNode column-major (x of node n at [3(n-1)]);
 *   - nodal vectors are 3nNode with dof = 3(n-1)+c;
 *   - integ_stress/integ_strain are 6 x 8nElement column-major, Voigt (xx,yy,zz,xy,yz,xz),
 *     Gauss point index 8(e-1)+i;  integ_* scalars are 8nElement;  Qe is 24 x nElement.
 * The library owns all device memory and converts layout (Julia AoS <-> device SoA, int64 1-based
 * <-> int32 0-based) at upload/download; it never frees caller memory.
 * Errors: every int-returning call returns 0 on success and a negative code on failure;
 * hakai_last_error() gives the message (thread-local). A context is used by one host thread.
 * There is no CPU fallback: compute entry points fail with HAKAI_ERR_DEVICE when no gfx950 device
 * is present.
 */
#ifndef HAKAI_HIP_H
#define HAKAI_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HAKAI_ABI_VERSION 1

enum {
    HAKAI_OK = 0,
    HAKAI_ERR_ARG = -1,      /* bad argument / shape */
    HAKAI_ERR_DEVICE = -2,   /* no device, HIP failure */
    HAKAI_ERR_IO = -3,       /* file open / parse */
    HAKAI_ERR_STATE = -4,    /* call order (e.g. step before upload_model) */
    HAKAI_ERR_MODEL = -5,    /* a case the reference itself rejects (e.g. 1-row *Plastic -> BoundsError) */
    HAKAI_ERR_COMM = -6      /* RCCL */
};

typedef struct hakai_ctx hakai_ctx;

/* One material as readInpFile builds it (MaterialType, v2/readInpFile_j.jl:84-96). G, Dmat
 * (v2/HAKAI_j.jl:143-160) and Hd (v2/readInpFile_j.jl:763-768) are derived inside. */
typedef struct {
    double density, young, poisson;
    int32_t n_plastic;      /* rows of *Plastic (yield stress, eq. plastic strain); 0 = elastic */
    const double* plastic;  /* row-major [n_plastic][2] */
    int32_t n_ductile;      /* rows of *Damage Initiation, criterion=DUCTILE; 0 = no deletion */
    const double* ductile;  /* row-major [n_ductile][3] (fracture strain, triaxiality, rate) */
} hakai_material_t;

/* Boundary conditions, flattened BCType list (v2/readInpFile_j.jl:98-104, :843-957).
 * Group g is one *Boundary block; its entries are (dof list, value) lines applied in order, later
 * groups overwrite earlier ones (v2/HAKAI_j.jl:585-617). amp_n[g] == 0 means no amplitude. */
typedef struct {
    int32_t n_groups;
    const int32_t* amp_n;      /* [n_groups] */
    const int64_t* amp_off;    /* [n_groups] into amp_time / amp_value */
    const double* amp_time;
    const double* amp_value;
    const int64_t* entry_off;  /* [n_groups+1] */
    const double* entry_value; /* [n_entries] */
    const int64_t* dof_off;    /* [n_entries+1] into dofs */
    const int64_t* dofs;       /* 1-based dofs */
} hakai_bc_t;

/* Per-step state in the reference layout (v2/HAKAI_j.jl:225-230, :430-456). Any pointer may be
 * NULL to skip that array. velo is derived (d_disp/d_time, :628) on download. */
typedef struct {
    double* disp;                    /* 3nN */
    double* disp_pre;                /* 3nN */
    double* velo;                    /* 3nN */
    double* Q;                       /* 3nN, internal force of the last step (used by the next) */
    double* integ_stress;            /* 6 x 8nE */
    double* integ_strain;            /* 6 x 8nE */
    double* integ_yield_stress;      /* 8nE */
    double* integ_eq_plastic_strain; /* 8nE */
    double* integ_triax_stress;      /* 8nE */
    int64_t* element_flag;           /* nE (1 = active, 0 = deleted) */
    double* Qe;                      /* 24 x nE element internal forces of the last step (:1330-1340) */
} hakai_state_t;

/* ---- library / device --------------------------------------------------------------------- */
int hakai_abi_version(void);
const char* hakai_last_error(void);
/* Number of visible HIP devices (0 on a host without GPU). */
int hakai_device_count(int* n);

/* ---- persistent device context (replaces the Julia-side state of hakai(), v2/HAKAI_j.jl:81-480) */
int hakai_create(hakai_ctx** ctx, int device);
int hakai_destroy(hakai_ctx* ctx);

/* Model: mesh, materials, lumped mass (diag_M is per dof, 3nN, as v2/HAKAI_j.jl:202-215 builds
 * it; the three dofs of a node must carry the same mass, as the reference always produces). */
int hakai_upload_model(hakai_ctx* ctx, int64_t nNode, const double* coordmat, int64_t nElement,
                       const int64_t* elementmat, const int64_t* element_material, int32_t nMat,
                       const hakai_material_t* mats, const double* diag_M);
int hakai_set_bc(hakai_ctx* ctx, const hakai_bc_t* bc);

/* Fresh state on device: disp = disp_pre = Q = 0, stress/strain/eqps/triax = 0, element_flag = 1,
 * yield = first *Plastic row (v2/HAKAI_j.jl:225-239, :430-465), then the initial velocity field
 * (ic_dofs 1-based, one value per dof): disp_pre[dof] = -v*d_time, velo[dof] = v (:233-239). */
int hakai_reset_state(hakai_ctx* ctx, int64_t n_ic, const int64_t* ic_dofs, const double* ic_values,
                      double d_time);
int hakai_upload_state(hakai_ctx* ctx, const hakai_state_t* st);
int hakai_download_state(hakai_ctx* ctx, hakai_state_t* st);

/* n_steps iterations of the time-loop body v2/HAKAI_j.jl:497-764 (with contact if enabled) for
 * t = t_first .. t_first+n_steps-1 (t is Float64 like `for t = 1:time_num`). Asynchronous with
 * respect to the host until hakai_sync / a download. */
int hakai_step(hakai_ctx* ctx, double t_first, int64_t n_steps, double d_time);
/* Launch-bound step loops run from hipGraphs: hakai_step captures `graph` steps per graph
 * (default 16, an even count; tuning key "graph" or env HAKAI_GRAPH, 0 = no capture), one graph per
 * starting parity, reused for the whole run, plus 2-step graphs for a run's tail. A step is captured
 * whenever it is the same launch sequence every time -- no multi-GPU exchange, no profiling, no
 * uploaded Q, contact in its steady state -- and the call's last step always runs in stream mode.
 * Results are bit-identical to stream mode. hakai_graph_steps returns the steps run from graphs. */
int hakai_graph_steps(hakai_ctx* ctx, int64_t* n_steps);
/* Step-loop counters (tests, tools; no reference counterpart): "graph_steps", "own_steps" (element
 * steps with owner-computed assembly), "own_rows" / "own_entries" (its exported rows / per-batch
 * entries for this mesh), "own_superbatch" (batches of 32 elements per LDS summing pass: 2, or 1
 * for wide meshes), "own_slots" (LDS running sums a block keeps open at most), "own_banded" (1: the
 * blocks walk row bands of a structured wide cross-section), "own_grid" (blocks of that schedule),
 * "own_round2" (summing passes that take a second entry per thread), "conn_patterns" (offset patterns
 * of the connectivity templates the element kernel reads; 0: it reads the plain connectivity array),
 * "conn_bytes" (connectivity bytes the element kernel reads per launch in that form),
 * "exchange_retries" (steps run again after a multi-GPU contact exchange block overflowed),
 * "device_buffers" (device arrays the library holds now, over every context of the process: equal
 * before a context's creation and after its destruction). */
int hakai_stat(hakai_ctx* ctx, const char* key, int64_t* value);
int hakai_sync(hakai_ctx* ctx);
/* Deletions so far (v2/HAKAI_j.jl:733-736): count, and up to cap (step, element 1-based) pairs. */
int hakai_deleted(hakai_ctx* ctx, int64_t* n_deleted, int64_t* log, int64_t cap);
/* Gauss points of active elements with det J < 0 in the current configuration (the reference
 * prints a warning and takes |det J|, :1736-1739). Diagnostic, runs a separate kernel. */
int hakai_negative_jacobians(hakai_ctx* ctx, int64_t* n);

/* GP -> node averages for output, on device (cal_node_stress_strain, v2/HAKAI_j.jl:3408-3486).
 * node_stress/node_strain are nN x 6 row-major; any pointer may be NULL. The divisor is the node's
 * number of incidences; the reference's (:3458) counts an element that lists a node twice once, so
 * the two differ only for such an element, which none of the committed decks has. */
int hakai_node_stress_strain(hakai_ctx* ctx, double* node_stress, double* node_strain,
                             double* node_eq_plastic_strain, double* node_mises_stress,
                             double* node_triax_stress);

/* ---- stateless literal drop-ins (host arrays, reference layout, in place; PCIe-bound, for parity) */
/* cal_stress_hexa(Qe, integ_stress, integ_strain, integ_yield_stress, integ_eq_plastic_strain,
 *   position, d_disp, elementmat, element_flag, integ_num, Pusai_mat, MATERIAL, element_material,
 *   elementMinSize, elementVolume)  -- v2/HAKAI_j.jl:1033-1036 (called at :664-667).
 * Qe is accumulated into (the reference zeroes it first at :662); integ_num must be 8;
 * Pusai_mat and elementMinSize are implied (the kernel builds Pusai in registers). */
int hakai_stress_hexa(int device, int64_t nNode, int64_t nElement, double* Qe, double* integ_stress,
                      double* integ_strain, double* integ_yield_stress, double* integ_eq_plastic_strain,
                      const double* position, const double* d_disp, const int64_t* elementmat,
                      const int64_t* element_flag, int32_t integ_num, int32_t nMat,
                      const hakai_material_t* mats, const int64_t* element_material, double* elementVolume);
/* cal_triax_stress(integ_stress, integ_triax_stress) -- v2/HAKAI_j.jl:982 (called at :677). */
int hakai_triax_stress(int device, int64_t nGP, const double* integ_stress, double* integ_triax_stress);

/* ---- host-side setup helpers (no GPU) ------------------------------------------------------ */
/* Element volumes and lumped mass, v2/HAKAI_j.jl:183-218 (diag_M per dof, 3nN). */
int hakai_lumped_mass(int64_t nNode, const double* coordmat, int64_t nElement, const int64_t* elementmat,
                      const int64_t* element_material, int32_t nMat, const hakai_material_t* mats,
                      double mass_scaling, double* diag_M, double* elementVolume);

/* ---- profiling: per-kernel device time measured with HIP events on the context's stream ---- */
/* HAKAI_K_CONTACT: the contact step (multi-GPU contact: phases A1-A3, the search); HAKAI_K_CONTACT_SUM:
 * multi-GPU contact phase B (the gathered events' force sums of the rank's nodes). */
enum { HAKAI_K_ELEMENT = 0, HAKAI_K_NODAL = 1, HAKAI_K_BC = 2, HAKAI_K_EXCHANGE = 3, HAKAI_K_CONTACT = 4,
       HAKAI_K_CONTACT_SUM = 5, HAKAI_K_COUNT = 6 };
int hakai_profile_enable(hakai_ctx* ctx, int on);  /* all kernels on / off; resets the totals */
/* Time only the kernels whose bit (1 << HAKAI_K_*) is set (fewer events in a timed loop). */
int hakai_profile_mask(hakai_ctx* ctx, uint32_t mask);
int hakai_profile_read(hakai_ctx* ctx, int kernel, double* total_ms, int64_t* launches);
/* Tuning knobs (results are bit-identical across every setting except elem_exact, which selects
 * the arithmetic):
 *   "elem_exact"        1: reference-order element arithmetic (cal_stress_hexa op for op; GPU
 *                       trajectories bit-identical to the reference's expression order; the mode
 *                       hakai_run_inp uses), 0 (default for hakai_step): fused single-pass element
 *                       kernel (rounding-level differences); env HAKAI_ELEM_EXACT sets the default;
 *   "elem_pipe_blocks"  >0: persistent software-pipelined element kernel on that many blocks
 *                       (default 512); 0: one batch of 32 elements per block;
 *   "elem_pipe_min"     persistent kernel only with >= this many batches per block (default 2);
 *   "elem_gp_nt"        1 (default): Gauss-point state streamed with nontemporal loads and stores;
 *   "own_assembly"      1 (default; env HAKAI_OWN_ASSEMBLY): the persistent element kernel sums node
 *                       forces in LDS in element order and hands the nodal update Q (+ the rows of
 *                       nodes shared between blocks) instead of the per-element force array; meshes
 *                       it does not fit use that array (hakai_stat "own_steps"), and so does the
 *                       reference-order kernel where the lists need two entries per thread in some
 *                       pass (wide sections, hakai_stat "own_round2": the array is faster there);
 *                       2: the owner sums wherever they fit;
 *   "own_band_rows"     0 (default): the banded owner schedule plans its row-band height; >0: that
 *                       height (capped by the block's LDS slots), re-planned at the next step;
 *   "own_pass_batches"  0 (default): owner summing passes over 2 batches where the lists fit, else 1;
 *                       1 or 2: that many (re-planned at the next step);
 *   "own_templates"     1 (default): the owner entry lists in template form where the plan offers one
 *                       -- each distinct summing pass stored once with relative targets, a 16-byte
 *                       header per pass (hakai_stat "own_templates": distinct passes, 0 = plain
 *                       form; "own_entries_stored"); 0: the plain lists; re-planned at the next step;
 *   "conn_templates"    1 (default): where the mesh has at most 256 distinct patterns of node offsets
 *                       conn[e][k] - conn[e][0] (a structured or extruded mesh has a handful), the
 *                       owner-assembly template variants of the fused element kernel read a 4-byte record
 *                       per element -- base node and pattern id -- and the cached pattern table
 *                       instead of the 32-byte connectivity row (hakai_stat "conn_patterns",
 *                       "conn_bytes"); other meshes and kernels read the plain array; 0: the plain
 *                       array everywhere;
 *   "nodal_padded"      0: CSR force gather instead of the padded [nN][8] table;
 *   "fuse_bc"           1 (default): one GPU, <= 2^18 nodes: the nodal kernel applies the BCs;
 *   "graph"             steps per captured hipGraph (even, default 16; 0 = stream mode);
 *   "history_one_block" history output's reduction: -1 (default) one launch up to 2048 nodes, two
 *                       above; 0: two launches; 1: one (the same bits either way);
 *   "elem_history_one_block" the element-set history's reduction: -1 (default) one launch up to 256
 *                       elements, two above; 0: two launches; 1: one (the same bits either way);
 *   "contact_event_cap", "contact_candidate_cap", "contact_full_rebuild": contact buffers and
 *                       rebuild policy;
 *   "contact_exchange_deletions", "contact_exchange_bins", "contact_exchange_events": multi-GPU
 *                       contact, records per rank block of each per-step exchange (they also grow
 *                       on their own; call on every rank between steps);
 *   "contact_fuse_small" 1 (default): decks of <= 2^16 elements run fused single-workgroup phases;
 *   "contact_fuse_binfilter" 1 (default): the binning (multi-GPU: the bucket insert) and the
 *                       triangle prefilter run in one launch, side by side;
 *   "group_serial"      1 on rank 0 of a hakai_step_group: each rank's phase is drained before the
 *                       next rank's (uncontended per-rank timings on one GPU; default 0); 2: the
 *                       same, each phase enqueued behind a fixed ≈0.3 ms sleep kernel so it runs
 *                       back to back on the GPU instead of at the host's enqueue pace. */
int hakai_set_tuning(hakai_ctx* ctx, const char* key, int64_t value);

/* ---- history output: per-step sums over node sets, computed on the device inside the step ---- */
/* With history enabled every hakai_step (captured graphs included) sums, after its nodal update
 * and BCs, 16 values over each node set -- set 0 is every node, sets 1..n_sets the caller's; a node
 * may be in several. Notation: u_k the displacement after k steps, Q_k / f_k the internal / contact
 * force assembled from u_k (what step k+1's nodal update consumes), du_k = u_k - u_{k-1},
 * c_k = (du_{k+1} + du_k) / 2. Step t = k+1 sums, per set:
 *    0-2  F_int[c]  Q_k (the reaction force on a clamped set)
 *    3-5  F_ext[c]  f_k (0 without contact, loads and walls; with hakai_set_loads / hakai_set_walls the
 *                   step's total external force, contact plus loads plus walls, so W_ext is their
 *                   work and the identity below holds)
 *    6-8  P[c]      m du_{k+1} / dt
 *    9    KE        1/2 m sum_c (du_{k+1} / dt)^2 (the velocity a download after this step reports)
 *   10    W_int     accumulated since the (re)start: += sum_c Q_k c_k
 *   11    W_ext     accumulated: += sum_c f_k c_k
 *   12    W_bc      accumulated, prescribed dofs only: += r_k c_k, the constraint force
 *                   r_k = m (du_{k+1} - du_k) / dt^2 + Q_k - f_k
 *   13-15 U[c]      u_k (a sum: divide by the set's size for the mean)
 * For set 0, KE - KE_seed + W_int - W_ext - W_bc = 0 up to rounding: an identity of the central
 * difference update (DESIGN.md "History output"), so its drift is a check of the whole step. The
 * works accumulate every step; a record (k, then the values of every set) is kept when
 * k % stride == 0, in a ring of the newest `capacity` records. Records describe states 0 .. N-1 of
 * an N-step run: the Q of the state after the last step is never consumed. The (re)start is the
 * enable call and every hakai_reset_state / hakai_upload_state: the count returns to 0, the works to
 * 0, and the first step afterwards stores KE_seed = sum 1/2 m ((disp - disp_pre) / d_time)^2 with
 * its d_time. A step a contact overflow poisoned leaves no record and accumulates nothing. The sums
 * are taken in a fixed tree over the node numbers: the same bits for every tuning setting and
 * launch form. hakai_upload_model disables history; hakai_set_bc keeps it.
 * Tuning "history_one_block" (-1 default: by mesh size; 0; 1) picks the reduction's launch form:
 * one workgroup in one launch, or chunk partials and a combining launch.
 *
 * On N ranks (a context with a communicator, hakai_comm_init / hakai_comm_init_local) every rank
 * keeps a PARTIAL record: the same sums, in the same tree over the rank's local node numbers, taken
 * over the nodes the rank owns. A node shared by ranks r and r+1 is owned by r (the contact search's
 * owner rule), so a rank owns every local node except those it shares with the rank below; a node
 * it does not own counts in no set, set 0 included. Each rank has its own ring and its own work
 * accumulators and nothing is exchanged per step. The record of the whole model is the sum of the
 * ranks' records in rank order, ((p_0 + p_1) + p_2) + ..., formed on the host by
 * hakai_history_combine; the same holds for KE_seed, and the works are linear, so the sum of the
 * ranks' accumulators is the accumulated work and the identity above holds for the combined set 0.
 * A one-GPU tree's chunks straddle the cuts, so the combined record is NOT the one-GPU record bit for
 * bit; it is deterministic for a given partition (the same bits for every tuning setting, both
 * launch forms, an in-process group and RCCL ranks) and within the same rounding bound of the exact
 * sums. On a rank: hakai_history_enable needs hakai_set_interface first (an empty interface counts;
 * without it HAKAI_ERR_STATE), set_nodes are the rank's local 1-based ids (both ranks may list a
 * shared node, only the owner counts it), stride and capacity must be the same on every rank, and
 * the call is collective like the state calls (every rank, in any order). hakai_comm_init,
 * hakai_comm_init_local and hakai_set_interface refuse a context with history enabled
 * (HAKAI_ERR_STATE: disable it first). hakai_history_count / hakai_history_read on a rank return
 * that rank's partial records. A step that a multi-GPU contact exchange overflow poisoned leaves no
 * record on any rank; the call runs it again. */
#define HAKAI_HISTORY_MAX_SETS 15
#define HAKAI_HISTORY_FIELDS 16
/* set_off[n_sets+1] into set_nodes (1-based node ids; duplicates within a set are an error; an
 * empty set is allowed and records zeros). Bad arguments (a node id out of range, more than 15
 * sets, stride < 1, capacity < 1) return HAKAI_ERR_ARG and change nothing. */
int hakai_history_enable(hakai_ctx* ctx, int32_t n_sets, const int64_t* set_off, const int64_t* set_nodes,
                         int64_t stride, int64_t capacity);
int hakai_history_disable(hakai_ctx* ctx);
/* records written since the last (re)start, and how many of the newest the ring still holds */
int hakai_history_count(hakai_ctx* ctx, int64_t* n_written, int64_t* n_held);
/* syncs; records [first, first+n) counted from the (re)start, must still be held (else
 * HAKAI_ERR_ARG); steps[n], values[n][(n_sets+1)][16], ke_seed[n_sets+1] (any pointer may be NULL) */
int hakai_history_read(hakai_ctx* ctx, int64_t first, int64_t n, int64_t* steps, double* values, double* ke_seed);
/* Host helper (no GPU): n records as CSV -- one header line step,time,<set>_<field>,... (fields
 * F_int_x .. U_z in record order, set_names[n_names] with set 0 first), one line per record with
 * time = step * d_time and every value as %.17g (parses back to the same double). */
int hakai_history_write_csv(const char* path, int32_t n_names, const char* const* set_names, int64_t n,
                            const int64_t* steps, const double* values, double d_time);
/* Host helper (no GPU): the ranks' partial records into the record of the whole model. Inputs in
 * rank order, as hakai_history_read returned them for the same [first, first+n) on every rank:
 * steps[n_ranks][n], values[n_ranks][n][n_total][16], ke_seed[n_ranks][n_total], with n_total =
 * n_sets + 1. Outputs steps_out[n], values_out[n][n_total][16], ke_seed_out[n_total]: every value is
 * ((p_0 + p_1) + p_2) + ... over the ranks, one rounding per addition; one rank is the identity.
 * HAKAI_ERR_ARG: a null array (steps, values and their outputs may be NULL only when n == 0),
 * n_ranks < 1, n_total outside 1..16, n < 0. HAKAI_ERR_STATE: the ranks' step numbers differ. A
 * refused call leaves the outputs untouched. */
int hakai_history_combine(int32_t n_ranks, int32_t n_total, int64_t n, const int64_t* steps, const double* values,
                          const double* ke_seed, int64_t* steps_out, double* values_out, double* ke_seed_out);

/* ---- element-set history: volume, mean stress and strain, energy split per element set -------- */
/* The element side of a history: functions of the Gauss-point state and the current geometry,
 * evaluated only at record steps by kernels of their own (nothing a step computes changes: the
 * trajectory is the same bits with the feature on and off). Set 0 is every element, sets 1..n_sets
 * the caller's; an element may be in several. An element counts as active if element_flag == 1;
 * every sum and extreme runs over the active elements of the set. With x = coord + u_k,
 * a_k = |det(P_k x^T)| at Gauss point k (the cal_Pusai_hexa table; hakai_stable_dt's determinant),
 * a0_k the same on coord, and sigma, eps (xx, yy, zz, xy, yz, zx), eqps the stored state:
 *    0     N_active      as a double
 *    1     N_deleted     elements of the set whose deletion step is non-zero
 *    2     V             sum a_k
 *    3     V0            sum a0_k
 *    4-9   S[c]          sum a_k sigma_k[c] (the mean stress is S / V, formed by the reader)
 *   10-15  E[c]          sum a_k eps_k[c]
 *   16     EQ            sum a_k eqps_k
 *   17     SE            sum a_k w_e(sigma_k), w_e = q^2 / (6 G) + p^2 / (2 K), p = tr sigma / 3, q the
 *                        Mises stress, K = (Dn + 2 Do) / 3: the recoverable strain energy
 *   18     PD            sum a0_k w_p(eqps_k), w_p the area under the material's piecewise linear
 *                        hardening curve (yield0 at the first row, the last slope continued beyond
 *                        the last row, 0 for an elastic material): the plastic dissipation.
 *                        Reference weights, because plastic flow is isochoric
 *   19,20  eqps_max      the largest eqps_k and the global 1-based id of its element (the lowest id
 *                        among equals); both 0 for a set without active elements
 *   21,22  mises_max     the largest q_k and its element, the same rule
 *   23     J_min         min over elements of V_e / V0_e; +inf for a set without active elements
 * SE + PD is not W_int of hakai_history: the radial return takes H from the segment at the start
 * of the increment, the stress update carries no rotation, the volume changes, and a deleted
 * element's energy leaves the sums (eroded energy is not tracked). DESIGN.md "Element-set history"
 * has the measured gap.
 * With the history enabled, step t = k+1 writes -- after its nodal update and BCs, before its
 * element update, when k % stride == 0 -- the record (k, values) of state k into a ring of the
 * newest `capacity` records. Records describe states 0 .. N-1 of an N-step run; the probe gives the
 * state after the last step. hakai_reset_state and hakai_upload_state return the count to 0;
 * hakai_upload_model disables the feature; hakai_set_bc, loads, walls and mass scaling leave it
 * alone (there are no accumulators). A step a contact overflow poisoned leaves no record. Enable and
 * disable drop captured step graphs. It is independent of hakai_history: either, both or neither.
 * The sums are taken in a fixed tree over the element numbers (8 elements of a wave, 4 waves of a
 * 32-element chunk, then chunks pairwise in order): the same bits for every tuning setting and for
 * both launch forms, tuning "elem_history_one_block" (-1 default: one workgroup in one launch up to
 * 256 elements, else chunk partials and a combining launch; 0; 1). Counts, extremes and ids are
 * exact.
 * On N ranks every element belongs to one rank: a rank's record is its partial over its local
 * elements (set ids are the rank's local 1-based ids, the recorded ids global: element offset +
 * local id), nothing is exchanged, no interface is needed, and hakai_elem_history_combine forms the
 * record of the whole model. Its counts, extremes and ids equal the one-GPU record's; its sums are
 * within the same rounding bound but not the same bits (the tree runs over local numbers). */
#define HAKAI_ELEM_HISTORY_MAX_SETS 15
#define HAKAI_ELEM_HISTORY_FIELDS 24
/* set_off[n_sets+1] into set_elems (1-based element ids; an empty set is allowed and records zeros,
 * 0 and +inf). HAKAI_ERR_ARG, and nothing changes: an id out of range, a duplicate within a set,
 * more than 15 sets, stride < 1, capacity < 1. HAKAI_ERR_STATE without a model. */
int hakai_elem_history_enable(hakai_ctx* ctx, int32_t n_sets, const int64_t* set_off, const int64_t* set_elems,
                              int64_t stride, int64_t capacity);
int hakai_elem_history_disable(hakai_ctx* ctx);
/* records written since the last (re)start, and how many of the newest the ring still holds */
int hakai_elem_history_count(hakai_ctx* ctx, int64_t* n_written, int64_t* n_held);
/* syncs; records [first, first+n) counted from the (re)start, must still be held (else
 * HAKAI_ERR_ARG); steps[n], values[n][(n_sets+1)][24] (either pointer may be NULL) */
int hakai_elem_history_read(hakai_ctx* ctx, int64_t first, int64_t n, int64_t* steps, double* values);
/* The record of the CURRENT state, off the step loop (like hakai_stable_dt: it needs a state, runs
 * on the context's stream, synchronises, writes only its own scratch and leaves captured graphs
 * valid; the steps before and after it are the same bits with and without it), with sets of its own:
 * values[(n_sets+1)][24]. per_elem (optional): [nElement][20] = V, V0, S[6], E[6], EQ, SE, PD,
 * eqps_max, q_max, V / V0 of every active element, zeros for the others. It works whether or not
 * the in-step history is enabled. HAKAI_ERR_ARG as for enable. */
int hakai_elem_history_probe(hakai_ctx* ctx, int32_t n_sets, const int64_t* set_off, const int64_t* set_elems,
                             double* values, double* per_elem);
/* Host helper (no GPU): n records as CSV -- one header line step,time,<set>_<field>,... (fields
 * N_active, N_deleted, V, V0, S_xx, S_yy, S_zz, S_xy, S_yz, S_zx, E_xx .. E_zx, EQ, SE, PD, eqps_max,
 * eqps_max_elem, mises_max, mises_max_elem, J_min; set_names[n_names] with set 0 first), one line
 * per record with time = step * d_time and every value as %.17g (parses back to the same double). */
int hakai_elem_history_write_csv(const char* path, int32_t n_names, const char* const* set_names, int64_t n,
                                 const int64_t* steps, const double* values, double d_time);
/* Host helper (no GPU): the ranks' partial records into the record of the whole model. Inputs in
 * rank order: steps[n_ranks][n], values[n_ranks][n][n_total][24], n_total = n_sets + 1. Fields 0-18
 * are added in rank order, ((p_0 + p_1) + p_2) + ..., one rounding per addition; 19-22 take the
 * larger value and the lower id among equals (a rank without active elements in the set holds 0, 0
 * and never wins against one with); 23 takes the smaller value. One rank is the identity.
 * HAKAI_ERR_ARG: a null array (may be NULL only when n == 0), n_ranks < 1, n_total outside 1..16,
 * n < 0. HAKAI_ERR_STATE: the ranks' step numbers differ. A refused call leaves the outputs
 * untouched. */
int hakai_elem_history_combine(int32_t n_ranks, int32_t n_total, int64_t n, const int64_t* steps,
                               const double* values, int64_t* steps_out, double* values_out);

/* ---- stable time step: per-element estimate and lower bound, reduced on the device ----------- */
/* The reference takes its step from the deck (v2/HAKAI_j.jl:112-116) and never checks it against the
 * mesh. hakai_stable_dt evaluates, for every active element (element_flag == 1) at the CURRENT
 * configuration x = coord + disp, two numbers and reduces them on the device (a separate kernel; it
 * needs a state, runs on the context's stream, synchronises, and writes nothing a step reads: the
 * steps before and after it, captured graphs included, are the same bits with and without it).
 * With P_k the cal_Pusai_hexa table at Gauss point k, J_k = P_k x^T, a_k = |det J_k|,
 * G_k = J_k^-1 P_k, V = sum_k a_k, V0 = sum_k det(P_k coord^T) (the volume hakai_lumped_mass forms),
 * rho' = density * mass_scaling, M = E (1 - nu) / ((1 + nu)(1 - 2 nu)), Kb = E / (3 (1 - 2 nu)),
 * mu = E / (2 (1 + nu)):
 *   dt_est   the conventional estimate L / c: L = V / A_max (A_max the largest of the six face areas,
 *            each 1/2 |d1 x d2| of the face's diagonals), c = sqrt(M / rho'). What other codes
 *            print; NOT a bound in either direction (dense eigensolves: 0.36 .. 1.73 of the true
 *            critical step, 1.06 .. 1.20 on cube meshes at nu >= 0.3).
 *   dt_safe  2 sqrt(m_e / kappa), m_e = rho' V0 / 8, kappa = Kb V sum g~^2 + 2 mu sum_k a_k sum G_k^2
 *            with g~ = (sum_k a_k G_k) / V the B-bar mean gradient: kappa bounds the largest
 *            eigenvalue of the element's ELASTIC B-bar stiffness, so the minimum over the elements is
 *            a guaranteed lower bound of the linear critical step 2 / omega_max when diag_M is the
 *            lumped mass times mass_scaling (what every driver uploads). The plastic tangent is no
 *            stiffer; the PENALTY STIFFNESS OF CONTACT AND OF RIGID WALLS (hakai_set_walls) IS NOT
 *            COVERED. (DESIGN.md section 2,
 *            "Stable time step", has the derivation.)
 * An active element with V0 <= 0, V == 0 or A_max == 0 reports 0 for both; a deleted element reports
 * +inf and counts nowhere. The sums over the Gauss points are one fixed pairwise tree and the
 * minimum and the counts are exact, so the result is the same bits for every grid and on the host
 * (csrc/hakai_stable_dt_elem.hpp is the one definition). */
typedef struct {
    double dt_est;   int64_t element_est;    /* 1-based + the context's element offset; 0: no active element (dt = +inf) */
    double dt_safe;  int64_t element_safe;   /* equal values: the lowest element id */
    int64_t n_active, n_est_below, n_safe_below;   /* elements with dt < d_time; 0 when d_time <= 0 */
} hakai_stable_dt_t;
/* mass_scaling > 0 (the factor diag_M was built with), d_time the step to count against (<= 0: no
 * counts). dt_est_elem / dt_safe_elem: nElement values each in element order, or NULL. */
int hakai_stable_dt(hakai_ctx* ctx, double mass_scaling, double d_time, hakai_stable_dt_t* out,
                    double* dt_est_elem, double* dt_safe_elem);
/* Host helper (no GPU): the ranks' results into the whole model's -- the minimum over the ranks, an
 * equal value goes to the lowest element id (a rank without an active element, element 0, never
 * wins), the counts are summed. HAKAI_ERR_ARG: n_ranks < 1 or a null pointer. */
int hakai_stable_dt_combine(int32_t n_ranks, const hakai_stable_dt_t* parts, hakai_stable_dt_t* out);
/* Host helper (no GPU): n records as CSV, header
 * step,time,d_time,dt_est,element_est,dt_safe,element_safe,n_active,n_est_below,n_safe_below,
 * time = steps[i] * d_time, every double as %.17g (parses back to the same double; inf as "inf"). */
int hakai_stable_dt_write_csv(const char* path, int64_t n, const int64_t* steps, const hakai_stable_dt_t* rec,
                              double d_time);

/* ---- selective mass scaling: add element mass up to a target stable step ---------------------- */
/* The reference knows only *Fixed Mass Scaling, which multiplies every node's mass. hakai_mass_scale
 * adds mass only to the elements whose own dt_safe (above) is below a target, as much as brings it
 * there; the elementwise bound holds for any per-element masses, so dt_target is then provably stable
 * for the elastic stiffness. There is no reference counterpart: the definition is this text and
 * csrc/hakai_mass_scale_elem.hpp (one host/device header, compiled without contraction).
 * State: added_e >= 0, the mass added to each of element e's 8 nodes; 0 until a call raises it; it
 * survives the element's deletion (the reference never takes a deleted element's mass back).
 * A call applies, to every active element at the current configuration, with V, gg = sum g~^2,
 * ss = sum_k s_k, V0 and the material constants exactly as hakai_stable_dt forms them:
 *     kappa = (Kb V) gg + two_mu ss;   m0 = rho8 V0;   half = (0.5 dt_target) / safety
 *     a = kappa (half half) - m0;   cap = (max_factor - 1) m0;   a > cap: a = cap, "capped"
 *     added_new = a > added_prev ? a : added_prev
 * An element with V0 <= 0, V == 0 or a kappa that is not finite is "unfixable" and keeps its added
 * mass; a deleted element is untouched. Mass only grows; the same call at the same state changes no
 * bit and reports n_changed = 0. For safety <= 1 - 2^-40, every active element that is neither capped
 * nor unfixable then has dt_safe = 2 sqrt((m0 + added_new) / kappa) >= dt_target.
 * Nodal mass: M_n = M0_n + sum of added_e over the node's incidences in ascending (8e + i) order,
 * every addition rounded once, zeros included (an element that lists a node twice adds twice); M0 is
 * the uploaded mass, copied at the first call; M_n is always summed from it. Every kernel of a step
 * reads that mass (the nodal update, gravity and walls, history, contact). Mid-run the added mass
 * takes the node's velocity (momentum grows by dm v), and under gravity it has weight.
 * The call needs a state, runs on the context's stream and synchronises; it is callable at state 0
 * or between hakai_step calls. It writes the mass buffer in place: captured step graphs stay valid
 * and run with the new mass. A call that changed some element restarts an enabled history like a
 * state upload (KE and P change their meaning); so does a clear that removed mass.
 * hakai_stable_dt on a scaled context evaluates m0 + added_e (dt_est stretched by
 * sqrt((m0 + added_e) / m0)); unscaled elements keep their bits.
 * HAKAI_ERR_ARG (nothing changes, the scaling stays in force): mass_scaling or dt_target not positive
 * and finite, safety outside (0, 1], max_factor < 1 or NaN. HAKAI_ERR_STATE: no state; a context with
 * a communicator (a shared node needs the neighbour rank's elements: refused, never dropped).
 * hakai_upload_model clears the scaling; hakai_set_bc, hakai_reset_state and hakai_upload_state keep it. */
typedef struct {
    int64_t n_active;      /* active elements */
    int64_t n_scaled;      /* elements with added > 0 after the call (deleted ones included: their mass stays) */
    int64_t n_changed;     /* active elements whose added mass this call raised */
    int64_t n_capped, n_unfixable;   /* of the active elements */
    double max_factor_reached;       /* max (m0 + added) / m0 over the active elements with V0 > 0 (1 if none) */
    int64_t element_factor;          /* its element, 1-based + the element offset; equal values: the lowest id; 0: none */
    double mass_added;     /* sum_e 8 added_e in one fixed binary tree in element order: the same bits for every grid */
    double dt_safe;        /* the minimum of dt_safe over the active elements AFTER the call (+inf: none) */
    int64_t element_safe;
} hakai_mass_scale_t;
/* mass_scaling > 0 (the factor diag_M was built with), dt_target > 0, safety in (0, 1] (the drivers
 * take 0.9: a choice, not a measurement), max_factor >= 1 (+inf: no cap). */
int hakai_mass_scale(hakai_ctx* ctx, double mass_scaling, double dt_target, double safety, double max_factor,
                     hakai_mass_scale_t* out);
/* elem_added: nElement values (zeros without scaling) or NULL; diag_M: 3 nNode values, the mass the
 * steps read, per dof, or NULL. */
int hakai_mass_scale_get(hakai_ctx* ctx, double* elem_added, double* diag_M);
/* Restores the uploaded mass bit for bit and frees the scaling's state. */
int hakai_clear_mass_scale(hakai_ctx* ctx);

/* ---- external loads: nodal forces, gravity and follower face pressure ------------------------- */
/* The reference has no loads: nothing here has a counterpart in it. With loads set, every hakai_step
 * (captured graphs included) forms, in one launch after the contact search and before the nodal
 * update, the step's total external force: per node and component, every addition rounded once,
 *     the contact force of the step (+0.0 without contact)
 *   + the node's concentrated entries, value * amp, in list order
 *   + the gravity entries, mass[n] * (grav_accel[c] * amp), in list order (all three components)
 *   + the node's pressure contributions, in ascending order of the press_* index.
 * That total is what the nodal update, the multi-GPU interface fix and the history output take as
 * the external force (history's F_ext / W_ext are then contact plus loads). A node without any load
 * gets the contact force (or zero) unchanged. Without loads (and without rigid walls, hakai_set_walls
 * below, whose forces join this sum after the pressure contributions) nothing is launched or allocated.
 *
 * Amplitude tables: n_amp tables, table a holds amp_n[a] >= 2 rows (time, value) at amp_off[a]. A
 * load names a table by index; -1 is the constant 1. The value at ct = t * d_time (in a captured
 * graph (*t_rd + 1.0) * dt from the device step counter, the same expression) follows the rule of
 * the *Boundary amplitudes: the first segment j with time[j] <= ct <= time[j+1], linearly
 * interpolated; if none matches, the first segment extrapolated.
 * Concentrated loads: cload_dof (1-based dofs), cload_value, cload_amp; several entries on a dof add.
 * Gravity: grav_accel[3 n_grav] (magnitude times direction) acts on the whole model through the
 * uploaded diag_M, so a mass-scaled model keeps the acceleration.
 * Pressure: press_elem (1-based), press_face (1..6), press_value, press_amp. A follower load: it is
 * evaluated every step on the current configuration coord + disp (the displacement the nodal update
 * reads), and only while the face's element is active (element_flag == 1). Faces in terms of the
 * elementmat columns 1..8: S1 = 1-2-3-4, S2 = 5-8-7-6, S3 = 1-5-6-2, S4 = 2-6-7-3, S5 = 3-7-8-4,
 * S6 = 4-8-5-1; on a non-inverted element a positive pressure pushes every face into the element
 * (a unit cube's face gets -p A n_out in total). With corners x0..x3 in that order, (xi_a, eta_a) =
 * (-,-), (+,-), (+,+), (-,+), g1 = (-x0+x1+x2-x3)/4, g2 = (-x0-x1+x2+x3)/4, h = (x0-x1+x2-x3)/4:
 *     F_a = (p amp) [ g1 x g2 + (xi_a / 3) g1 x h + (eta_a / 3) h x g2 ],
 * the exact integral of N_a (dx/dxi x dx/deta); the four sum to p times the face's area vector.
 * csrc/hakai_loads_face.hpp is the one definition of the operation order.
 *
 * hakai_set_loads replaces the loads (the arrays are copied). HAKAI_ERR_ARG changes nothing and
 * leaves the previous loads in force: a dof or element out of range, a face outside 1..6, an
 * amplitude index out of range, a table with fewer than two rows, a non-finite value, a negative
 * count. HAKAI_ERR_STATE: before hakai_upload_model; pressure on a context with a communicator (a
 * face across a cut needs nodes the rank does not hold). On such a context concentrated loads and
 * gravity are accepted: every rank gives the full load of each of its local nodes, shared nodes
 * included, with local ids, and the result is bit-identical to one context.
 * hakai_upload_model clears the loads; hakai_set_bc, hakai_reset_state and hakai_upload_state keep
 * them. hakai_set_loads and hakai_clear_loads drop captured step graphs and, with history enabled,
 * restart the history like a state upload (W_ext changes its meaning).
 * hakai_load_force is a probe like hakai_contact_force: the load force (3nN, without contact) of
 * step t at the current state, no step; zeros without loads. */
typedef struct {
    int32_t n_amp;
    const int32_t* amp_n;       /* [n_amp] rows per table (>= 2) */
    const int64_t* amp_off;     /* [n_amp] into amp_time / amp_value */
    const double* amp_time;
    const double* amp_value;
    int64_t n_cload;
    const int64_t* cload_dof;   /* [n_cload] 1-based dofs */
    const double* cload_value;  /* [n_cload] */
    const int32_t* cload_amp;   /* [n_cload] table index, -1: constant 1 */
    int32_t n_grav;
    const double* grav_accel;   /* [3 n_grav] */
    const int32_t* grav_amp;    /* [n_grav] */
    int64_t n_press;
    const int64_t* press_elem;  /* [n_press] 1-based elements */
    const int32_t* press_face;  /* [n_press] 1..6 */
    const double* press_value;  /* [n_press] */
    const int32_t* press_amp;   /* [n_press] */
} hakai_loads_t;
int hakai_set_loads(hakai_ctx* ctx, const hakai_loads_t* loads);
int hakai_clear_loads(hakai_ctx* ctx);
int hakai_load_force(hakai_ctx* ctx, double t, double d_time, double* load_force);

/* ---- rigid walls: moving planes with penalty, damping and Coulomb friction -------------------- */
/* The reference has no rigid wall (its decks mesh a second body): the definition is this text. Up to
 * HAKAI_MAX_WALLS infinite planes. Wall w has
 *   origin[3], normal[3]  any finite non-zero normal; the host normalises it once,
 *                         n = normal / sqrt((nx*nx + ny*ny) + nz*nz), each component divided (a
 *                         length that is not finite and positive is refused). n points into the
 *                         half-space the nodes may occupy;
 *   motion[3], amp        the wall is rigid and displaced by motion * amp(tau); amp is an index into the
 *                         walls' own amplitude tables (layout and rule of hakai_loads_t's), -1 the
 *                         constant 1;
 *   stiffness >= 0 (force per length), scale >= 0: node i sees the penalty
 *                         k_i = stiffness + scale * (m_i / (dt * dt)), m_i the uploaded diag_M entry of
 *                         the node's first dof, so a mass-scaled model keeps its penalty ratio. An
 *                         isolated node on that spring alone is stable for scale < 4; the element
 *                         stiffness at the node shares that budget (and hakai_stable_dt's dt_safe does
 *                         not cover the wall): the choice is the caller's;
 *   damping >= 0 (zeta, fraction of critical), friction >= 0 (mu);
 *   nodes                 node_off[w] .. node_off[w+1] into nodes (1-based; local ids on a rank); an
 *                         empty range means every node; a node listed twice counts once.
 * Step t evaluates the force on the configuration its nodal update reads, u_k = disp, whose time is
 * tau0 = (t - 1.0) * d_time; with taum = (t - 2.0) * d_time, s0 = amp(tau0), sm = amp(taum) (in a captured
 * graph tau0 = (*t_rd) * dt and taum = (*t_rd - 1.0) * dt from the device step counter: the same bits),
 * u_km = disp_pre, m = m_i, dt = d_time, per component c and every operation rounded once:
 *     o[c]  = origin[c] + motion[c] * s0
 *     vw[c] = motion[c] * ((s0 - sm) / dt)
 *     x[c]  = coord[c] + u_k[c]
 *     v[c]  = (u_k[c] - u_km[c]) / dt - vw[c]
 *     g     = ((x[0] - o[0]) * n[0] + (x[1] - o[1]) * n[1]) + (x[2] - o[2]) * n[2]
 *     d     = -g
 * The wall acts only if d > 0 (strict: a node exactly on the plane gets nothing). Then
 *     k     = stiffness + scale * (m / (dt * dt))
 *     vn    = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]
 *     cd    = (2.0 * zeta) * sqrt(m * k)
 *     N     = max(k * d - cd * vn, 0.0)                       non-adhesive
 *     vt[c] = v[c] - vn * n[c]
 *     s     = sqrt((vt[0] * vt[0] + vt[1] * vt[1]) + vt[2] * vt[2])
 *     T     = min(mu * N, (m * s) / dt)                       the force that stops the slip in one step
 *     F[c]  = s > 0 ? N * n[c] - (T / s) * vt[c] : N * n[c]
 * csrc/hakai_walls_node.hpp is the one definition of this operation order, for the device and the host.
 * Place in the node's sum (hakai_set_loads above): after the pressure contributions, walls in
 * ascending index, each F added componentwise with one rounding per addition:
 *     contact (+0.0) + concentrated + gravity + pressure + walls,
 * formed in the same single launch as the loads; independent of grid, launch form and rank. The total
 * is what the nodal update, the interface fix and the history output take (history's F_ext / W_ext
 * carry the wall; the set-0 identity holds). Without walls and loads nothing is launched or allocated.
 *
 * hakai_set_walls replaces the walls (the arrays are copied); n_wall == 0 clears them. HAKAI_ERR_ARG
 * changes nothing and leaves the previous walls in force: more than HAKAI_MAX_WALLS walls or a
 * negative count, a node out of range, a zero or non-finite normal, a non-finite origin or motion,
 * a non-finite or negative stiffness, scale, damping or friction, an amplitude index out of range, a
 * table with fewer than two rows or a non-finite row. HAKAI_ERR_STATE: before hakai_upload_model.
 * A context with a communicator accepts walls: every rank lists each of its local nodes, shared ones
 * included, with local ids, and the result is bit-identical to one context.
 * hakai_upload_model clears the walls; hakai_set_bc, hakai_reset_state and hakai_upload_state keep
 * them. Loads and walls are independent: setting or clearing one leaves the other in force.
 * hakai_set_walls and hakai_clear_walls drop captured step graphs and, with history enabled, restart
 * the history. hakai_wall_force is a probe like hakai_load_force: the wall force alone (3nN, without
 * contact and loads) of step t at the current state, no step; zeros without walls. hakai_load_force
 * keeps returning the loads only, hakai_contact_force the contact only. */
#define HAKAI_MAX_WALLS 32
typedef struct {
    int32_t n_amp;
    const int32_t* amp_n;       /* [n_amp] rows per table (>= 2) */
    const int64_t* amp_off;     /* [n_amp] into amp_time / amp_value */
    const double* amp_time;
    const double* amp_value;
    int32_t n_wall;
    const double* origin;       /* [3 n_wall] */
    const double* normal;       /* [3 n_wall] */
    const double* motion;       /* [3 n_wall] */
    const int32_t* amp;         /* [n_wall] table index, -1: constant 1 */
    const double* stiffness;    /* [n_wall] */
    const double* scale;        /* [n_wall] */
    const double* damping;      /* [n_wall] */
    const double* friction;     /* [n_wall] */
    const int64_t* node_off;    /* [n_wall + 1] into nodes */
    const int64_t* nodes;       /* 1-based node ids; an empty range: every node */
} hakai_walls_t;
int hakai_set_walls(hakai_ctx* ctx, const hakai_walls_t* walls);
int hakai_clear_walls(hakai_ctx* ctx);
int hakai_wall_force(hakai_ctx* ctx, double t, double d_time, double* wall_force);

/* ---- contact: all-exterior instance-vs-instance penalty contact --------- */
/* Enables contact for the uploaded model: contact_flag as readInpFile sets it (1 = *Contact,
 * 2 = HAKAIoption=self-contact; v2/readInpFile_j.jl:1046-1060), element_instance = instance
 * (1-based, contiguous element blocks) of each element. Builds the exterior surfaces and pairs
 * (v2/HAKAI_j.jl:244-421, :1944-2164) and, once, every face an element deletion can expose
 * (:2167-2245, :766-804). Then every hakai_step
 * computes cal_contact_force (:2248-2706) into the external force before the nodal update. */
int hakai_set_contact(hakai_ctx* ctx, int32_t contact_flag, const int64_t* element_instance);
/* Same with explicit *Contact Pair surfaces (v2/readInpFile_j.jl:517-564, :1063-1102; pairs
 * v2/HAKAI_j.jl:273-345): pair k couples instances cp_instance[2k], cp_instance[2k+1] (1-based);
 * side s of pair k holds the surface's elements cp_elems[cp_elem_off[2k+s] .. cp_elem_off[2k+s+1])
 * (instance-local, 1-based). n_cp = 0 is the all-exterior case of hakai_set_contact. */
int hakai_set_contact_cp(hakai_ctx* ctx, int32_t contact_flag, const int64_t* element_instance, int32_t n_cp,
                         const int32_t* cp_instance, const int64_t* cp_elem_off, const int64_t* cp_elems);
/* Multi-GPU contact (same reference seams as hakai_set_contact_cp). Call on every
 * rank after hakai_comm_init[_local], hakai_set_element_offset and hakai_set_interface, with the
 * GLOBAL model (the arrays of hakai_upload_model / hakai_set_contact_cp for the whole mesh, and
 * its global diag_M), local_node_global[l] = global 1-based id of this rank's local node l, and
 * rank_elem_off[0..nranks] = the ranks' contiguous global element ranges (0-based, rank r holds
 * [rank_elem_off[r], rank_elem_off[r+1])). Owner-computed search: each rank keeps the triangles
 * of its elements and the contact nodes it owns (the rank of the node's lowest incident element);
 * per step the deletions are all-gathered, the pair boxes all-reduced (exact min/max), the own
 * contact-zone nodes binned and all-gathered, each rank searches its own triangles, and the events
 * are all-gathered; each rank sums the forces of its own nodes. The contact force is
 * bit-identical to one GPU. hakai_set_contact[_cp] on a rank with a communicator returns
 * HAKAI_ERR_STATE. hakai_step, hakai_reset_state, hakai_upload_state and
 * hakai_set_tuning("contact_exchange_*") are collective: every rank calls them in the same order.
 * An exchange capacity overflow grows the capacity and the step runs again (up to 8 times);
 * hakai_contact_force is refused on such a rank (step the group instead). */
int hakai_set_contact_global(hakai_ctx* ctx, int32_t contact_flag, int64_t nNode, const double* coordmat,
                             int64_t nElement, const int64_t* elementmat, const int64_t* element_material,
                             const int64_t* element_instance, const double* diag_M, const int64_t* local_node_global,
                             const int64_t* rank_elem_off, int32_t n_cp, const int32_t* cp_instance,
                             const int64_t* cp_elem_off, const int64_t* cp_elems);
/* The constants hard-coded at v2/HAKAI_j.jl:2255-2259 (defaults myu 0.25, kc_o 1, kc_s 1,
 * Cr_o 0, Cr_s 0). BASELINE's C4 runs frictionless: myu = 0. */
int hakai_set_contact_params(hakai_ctx* ctx, double myu, double kc_o, double kc_s, double Cr_o, double Cr_s);
/* Pairs (CT entries): info[5p..5p+4] = (i_instance, j_instance, #nodes_i, #triangles, #nodes_j)
 * at setup; sizes = (elementMinSize, elementMaxSize). */
int hakai_contact_info(hakai_ctx* ctx, int32_t* n_pairs, int64_t* info, int32_t cap, double* sizes);
/* Counters of the last contact step (diagnostics; syncs the stream): stats[0..cap) = events,
 * max events in any step, prefiltered triangles, nodes with contact force, live triangles, live
 * i-node entries, live j-node entries (the last three = the lengths of the reference's c_triangles,
 * c_nodes_i, c_nodes_j summed over pairs, deleted elements' triangles included); multi-GPU only:
 * [7] contact-zone nodes all ranks binned in the last step, [8] bytes this rank's exchanges receive
 * per step (the other ranks' deletion, bin and event blocks, each at its rank's capacity;
 * hakai_set_contact_global); [9] hash-grid buckets of all pairs; [10] live triangles the prefilter
 * tested in full in the last step (those whose pair has a non-empty range box; multi-GPU: this
 * rank's); [11] multi-GPU: bytes of the records in those blocks in the last step (headers + the
 * gathered counts), what [8] would be with blocks sized exactly. */
int hakai_contact_stats(hakai_ctx* ctx, int64_t* stats, int32_t cap);
/* Probe: the contact force (3nN, = external_force of step t) at the current state, no step. */
int hakai_contact_force(hakai_ctx* ctx, double t, double d_time, double* external_force);

/* ---- multi-GPU: one process per GPU, contiguous element ranges, RCCL over xGMI -------------- */
int hakai_comm_unique_id(uint8_t id[128]);
/* Attach a communicator (ncclCommInitRank) to a context created on this rank's device. */
int hakai_comm_init(hakai_ctx* ctx, int rank, int nranks, const uint8_t id[128]);
/* In-process group: contexts in one process that pass the same group_key exchange interface
 * forces with device copies instead of RCCL (several subdomains on one device; the same pack /
 * sum / fix kernels as the RCCL path). The host must step all ranks in lockstep (rank 0..n-1,
 * one hakai_step call of equal length each) on the same device: a context on another device than
 * the group's members is rejected with HAKAI_ERR_ARG (the group's kernels read the peers' buffers
 * directly; across devices use hakai_comm_init). */
int hakai_comm_init_local(hakai_ctx* ctx, int rank, int nranks, int64_t group_key);
/* Steps an in-process group (the n contexts of hakai_comm_init_local, ctxs[r] = rank r) in lockstep,
 * n_steps steps from t_first: per step every rank's contact phase A1 (deletions, live lists, boxes),
 * then every rank's A2 (box combine, binning), A3 (hash grid, triangle search), then every rank's
 * phase B (event sums), nodal and element update, so the multi-GPU contact search works in one
 * process. A contact rank of an in-process group cannot step alone (HAKAI_ERR_STATE). */
int hakai_step_group(hakai_ctx** ctxs, int32_t n, double t_first, int64_t n_steps, double d_time);
/* Interface description for this rank's local model ("multi-GPU"):
 * shared nodes (local 0-based ids, sorted by global id) with the rank range [lo, hi] of ranks
 * whose elements touch each node (hi == lo+1 for slab partitions). */
int hakai_set_interface(hakai_ctx* ctx, int64_t n_shared, const int64_t* local_node, const int32_t* rank_lo,
                        const int32_t* rank_hi);
/* Global id offset of this rank's element 0 (deletion log reports global 1-based ids). */
int hakai_set_element_offset(hakai_ctx* ctx, int64_t element_offset);

/* ---- driver surface: .inp reader, VTK writer, HAKAI(fname) ---------------------------------- */
/* Flattened ModelType (v2/readInpFile_j.jl:129-150) as the solver consumes it. Owned by the
 * library; free with hakai_inp_free. */
typedef struct {
    int64_t nNode;
    const double* coordmat;           /* 3 x nNode */
    int64_t nElement;
    const int64_t* elementmat;        /* 8 x nElement, 1-based */
    const int64_t* element_material;  /* nElement, 1-based */
    const int64_t* element_instance;  /* nElement, 1-based */
    int32_t nMat;
    const hakai_material_t* materials;
    double d_time, end_time, mass_scaling;
    int32_t contact_flag;             /* 0 none, 1 *Contact, 2 self-contact option */
    hakai_bc_t bc;
    int64_t n_ic_dofs;                /* initial velocity: dofs (1-based) and values, in IC order */
    const int64_t* ic_dofs;
    const double* ic_values;
    int32_t n_instance;
    const int64_t* instance_node_offset;    /* [n_instance] */
    const int64_t* instance_element_offset; /* [n_instance] */
    const int64_t* instance_nElement;       /* [n_instance] */
    int32_t n_cp;                           /* *Contact Pair blocks (0: all-exterior contact) */
    const int32_t* cp_instance;             /* [2 n_cp] instances (1-based) of the two surfaces */
    const int64_t* cp_elem_off;             /* [2 n_cp + 1] into cp_elems */
    const int64_t* cp_elems;                /* surface elements, instance-local 1-based */
    /* *Cload, *Dload (GRAV on the whole model, Pn on an element set) and *Dsload (P on a *Surface),
     * each with an optional amplitude=NAME; global ids; the arrays are owned by the model. A deck
     * without these keywords has every count 0. An unknown load type, surface, set or amplitude is a
     * parse error. */
    hakai_loads_t loads;
    /* *Rigid Wall, name=NAME [, nset=NAME] [, amplitude=NAME] [, stiffness=K] [, scale=S] [, damping=Z]
     * [, friction=MU], then one data line ox, oy, oz, nx, ny, nz [, mx, my, mz]: a HAKAI keyword (the
     * reference's reader skips keywords it does not know). Defaults: stiffness 0, scale 0.5, damping 0,
     * friction 0, no motion, every node; nset gives global ids. An unknown parameter, node set or
     * amplitude, a malformed or missing data line and a 33rd wall are parse errors. A deck without
     * the keyword has n_wall 0. */
    hakai_walls_t walls;
    /* *Variable Mass Scaling [, dt=TARGET] [, safety=S] [, max factor=F] [, repeat=output]: a HAKAI
     * keyword (the reference's reader skips it; the name does not contain "*Fixed Mass Scaling", whose
     * parse is untouched). The one-GPU drivers call hakai_mass_scale after hakai_reset_state and, with
     * repeat=output, again at every VTK output state before the next chunk of steps. Defaults: dt 0 (=
     * the stepped d_time, increment * sqrt(mass_scaling)), safety 0.9, max factor +inf (no cap), state
     * 0 only. An unknown parameter, a malformed value, dt <= 0, safety outside (0, 1], max factor < 1 or
     * a second keyword line are parse errors. A deck without the keyword has vms_set 0. */
    int32_t vms_set;        /* 1: the deck has the keyword */
    int32_t vms_repeat;     /* 1: repeat=output */
    double vms_dt;          /* the target; 0: the stepped d_time */
    double vms_safety;
    double vms_max_factor;
} hakai_inp_model_t;

int hakai_inp_read(const char* path, hakai_inp_model_t** out);
void hakai_inp_free(hakai_inp_model_t* m);

/* Legacy-ASCII VTK writer with the reference's content (write_vtk, v2/HAKAI_j.jl:3517-3717):
 * writes <dir>/file%03d.vtk. node arrays as produced by hakai_node_stress_strain. */
int hakai_write_vtk(const char* dir, int index, int64_t nNode, const double* coordmat, int64_t nElement,
                    const int64_t* elementmat, const int64_t* element_flag, const double* disp,
                    const double* velo, const double* node_stress, const double* node_strain,
                    const double* node_eq_plastic_strain, const double* node_mises_stress,
                    const double* node_triax_stress);

/* Asynchronous, multi-threaded VTK writer (same bytes as hakai_write_vtk). A writer holds the
 * mesh (initial coordinates are formatted once, elementmat is copied) and writes one file at a
 * time on a background thread, so the device keeps stepping while the previous output is
 * formatted (the reference writes synchronously, v2/HAKAI_j.jl:932-942). n_threads <= 0: env
 * HAKAI_VTK_THREADS, else OMP_NUM_THREADS, else all hardware threads (at most 64).
 *   submit: copies the arrays, waits for the file in flight, starts <dir>/file%03d.vtk.
 *   acquire/commit: zero-copy variant; acquire returns the writer's fill buffers (valid until
 *   commit), commit waits for the file in flight and starts writing the filled buffers.
 *   wait: blocks until the file in flight is written; returns its status (write errors of an
 *   earlier file also surface at the next submit/commit). destroy waits, then frees. */
typedef struct hakai_vtk_writer hakai_vtk_writer;
typedef struct {
    int64_t* element_flag;           /* nElement */
    double* disp;                    /* 3 x nNode */
    double* velo;                    /* 3 x nNode */
    double* node_stress;             /* 6 x nNode */
    double* node_strain;             /* 6 x nNode */
    double* node_eq_plastic_strain;  /* nNode */
    double* node_mises_stress;       /* nNode */
    double* node_triax_stress;       /* nNode */
} hakai_vtk_arrays_t;
int hakai_vtk_writer_create(hakai_vtk_writer** w, const char* dir, int64_t nNode, const double* coordmat,
                            int64_t nElement, const int64_t* elementmat, int n_threads);
int hakai_vtk_writer_submit(hakai_vtk_writer* w, int index, const int64_t* element_flag, const double* disp,
                            const double* velo, const double* node_stress, const double* node_strain,
                            const double* node_eq_plastic_strain, const double* node_mises_stress,
                            const double* node_triax_stress);
int hakai_vtk_writer_acquire(hakai_vtk_writer* w, hakai_vtk_arrays_t* arrays);
int hakai_vtk_writer_commit(hakai_vtk_writer* w, int index);
int hakai_vtk_writer_wait(hakai_vtk_writer* w);
void hakai_vtk_writer_destroy(hakai_vtk_writer* w);

/* HAKAI(fname) (v2/HAKAI_j.jl:81-978): read, set up, run the whole step loop on `device`, write
 * out_dir/file000.vtk .. file100.vtk every floor(time_num/100) steps. verbose=1 prints the
 * reference's progress lines. Returns 0 or <0.
 * Env HAKAI_HISTORY=<stride> (>= 1) enables history output for the run and writes
 * out_dir/history.csv (hakai_history_write_csv) at the end: set "all", then "inst<i>" per instance,
 * then "bc<g>" per *Boundary group (the nodes of its dofs), 15 sets at most (verbose: the ones left
 * out are named on stderr); the ring holds the whole run. Without the variable nothing changes.
 * A deck with *Variable Mass Scaling: hakai_mass_scale after the reset (and, with repeat=output, at
 * every VTK output state but the last, before HAKAI_DT_CHECK's evaluation of that state and the next
 * chunk of steps), one line per application in out_dir/mass_scale.csv: step,dt_target,n_active,n_scaled,
 * n_changed,n_capped,n_unfixable,mass_added,max_factor_reached,element_factor,dt_safe,element_safe
 * (doubles as %.17g); verbose: one stderr line per application that changed something.
 * Env HAKAI_DT_CHECK=1 records hakai_stable_dt at state 0 and at every VTK output (the deck's
 * mass_scaling, the stepped d_time = increment * sqrt(mass_scaling)) and writes
 * out_dir/stable_dt.csv (hakai_stable_dt_write_csv) at the end; verbose: one stderr line the first
 * time d_time > dt_est and one the first time d_time > dt_safe, each naming the element. The VTK
 * files and stdout are the same bytes with and without; unset, nothing changes.
 * Env HAKAI_ELEM_HISTORY=<stride> (>= 1, else HAKAI_ERR_ARG) enables the element-set history for the
 * run and writes out_dir/elem_history.csv (hakai_elem_history_write_csv) at the end: the in-step
 * records of the whole run plus one final hakai_elem_history_probe record for the last state. Sets:
 * "all", then "inst<i>" per instance, then "mat<j>" per material when nMat > 1, then the deck's
 * *Elset ... instance= sets as "<instance>.<elset>" in deck order, 15 at most (verbose: the ones left
 * out are named on stderr). Unset, every byte of output is as before. The N-GPU driver (hakai.run)
 * refuses to run with the variable set.
 * The deck's loads (hakai_inp_model_t::loads) are applied with hakai_set_loads, its rigid walls
 * (hakai_inp_model_t::walls) with hakai_set_walls. */
int hakai_run_inp(const char* fname, const char* out_dir, int device, int verbose);
/* The sets of that history output, for another driver of the same deck (the N-GPU driver, hakai.run):
 * n_sets (without set 0), set_off[n_sets+1] (room for 16) into set_nodes (global 1-based ids;
 * NULL: only the offsets, set_off[n_sets] is the room set_nodes needs), names: "all", the n_sets
 * kept names, then the n_dropped names left out, each ended by a newline (NULL: none).
 * HAKAI_ERR_ARG if nodes_cap or names_cap is too small. */
int hakai_inp_history_sets(const hakai_inp_model_t* model, int32_t* n_sets, int64_t* set_off, int64_t* set_nodes,
                           int64_t nodes_cap, char* names, int64_t names_cap, int32_t* n_dropped);
/* The sets of the element-set history output (HAKAI_ELEM_HISTORY), the contract of
 * hakai_inp_history_sets: n_sets (without set 0), set_off[n_sets+1] (room for 16) into set_elems (global
 * 1-based element ids, ascending; NULL: only the offsets), names: "all", the n_sets kept names, then
 * the n_dropped names left out, each ended by a newline (NULL: none). HAKAI_ERR_ARG if elems_cap or
 * names_cap is too small. The deck's *Elset sets live in the model's private storage. */
int hakai_inp_elem_history_sets(const hakai_inp_model_t* model, int32_t* n_sets, int64_t* set_off, int64_t* set_elems,
                                int64_t elems_cap, char* names, int64_t names_cap, int32_t* n_dropped);

#ifdef __cplusplus
}
#endif
#endif
