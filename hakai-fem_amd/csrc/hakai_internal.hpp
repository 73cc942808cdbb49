// hakai_internal.hpp -- context definition shared by the translation units of libhakai_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/hakai_hip.h"
#include "hakai_device.hpp"
#include "hakai_devmem.hpp"
#include "hakai_kernels.hpp"
#include "hakai_own.hpp"
#include "hakai_step_view.hpp"

namespace hkc {
struct Comm;     // multi-GPU state (hakai_comm.cpp)
struct Contact;  // contact search state (hakai_contact_state.hpp)
struct History;  // history output state (hakai_history.hip)
struct ElemHistory;  // element-set history state (hakai_elem_history.hip)
struct StableDt; // stable-time-step scratch (hakai_stable_dt.hip)
struct Loads;    // external loads and rigid walls (hakai_loads.hip)
struct MassScale; // selective mass scaling (hakai_mass_scale.hip)
int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
}  // namespace hkc

struct EventPair {
    hipEvent_t a, b;
    int kernel;
};


// BCs fused into k_nodal up to this many nodes: the per-node lookup (4 B/node, one dependent load)
// costs more than the k_bc launch it saves on large meshes (C3: nodal 0.165 -> 0.180 ms, measured
// profiles/r02_assembly_bound_sweep.log), and wins on launch-bound small decks. With owner-computed
// assembly it neither wins nor loses on C3 / the C5 slab (profiles/r03_fuse_bc_sweep.log).
constexpr long long kFuseBcMaxNodes = 1 << 18;

struct hakai_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // model
    long long nN = 0, nE = 0, nEp = 0, ld = 0;
    // Device memory: every array below is a hkc::DevBuf that this context owns (hakai_devmem.hpp); the
    // two raw pointers, d_fext and d_ftot, are views of arrays that another state owns.
    hkc::DevBuf<double> d_coord;
    hkc::DevBuf<double> d_u[2];           // d_u[sv.cur] = disp, d_u[1-sv.cur] = disp_pre
    hkc::StepView sv;            // the host's view of the stepping state (hakai_step_view.hpp)
    hkc::DevBuf<double> d_mass;
    hkc::DevBuf<int> d_conn;
    // connectivity templates (hakai_conn_plan.hpp), planned by hakai_upload_model: the element
    // kernel's packed records [nEp] followed by the offset table [conn_P][8]; conn_P 0: the mesh has no
    // compressed form
    hkc::DevBuf<unsigned> d_conn_rec;
    int conn_P = 0, conn_bits = 0;
    long long conn_bytes = 0;    // connectivity bytes per launch of the compressed form
    int conn_templates = 1;      // tuning "conn_templates": use the compressed form where it exists
    hkc::DevBuf<int> d_flag;
    hkc::DevBuf<int> d_mat;
    hkc::DevBuf<hk::DevMat> d_mats;
    std::vector<hk::DevMat> h_mats;
    bool has_ductile = false;
    hkc::DevBuf<double> d_stress, d_strain, d_eqps, d_yield, d_triax, d_fe;
    hkc::DevBuf<int> d_inc_ptr;
    hkc::DevBuf<int> d_inc;      // CSR incidences as force base offsets of the active layout
    hkc::DevBuf<int> d_inc_row;  // the same incidences as (8e+k), for element-indexed data
    hkc::DevBuf<int> d_inc8;     // padded incidence table, null if a node has > 8 incidences
    // Element forces [nEp][8][3] (= the reference's Qe column order), row (e, k) at base 24e + 3k;
    // d_inc / d_inc8 hold the bases, and base 24nEp is an all-zero row (padding).
    long long fe_len = 0;        // doubles allocated for fe
    int max_inc = 0;
    std::vector<int> h_ptr, h_inc0;  // CSR node -> (8e+k), ascending element order
    int pipe_blocks = 512;       // persistent pipelined element kernel grid (0 = simple kernel)
    int pipe_min = 2;            // persistent kernel only with >= pipe_min batches per block (small
                                 // meshes: one batch per block, the pipeline only adds latency)
    int gp_nt = 1;               // element kernel: Gauss-point state nontemporal (loads and stores)
    int elem_exact = 0;          // tuning "elem_exact": reference-order element arithmetic
    int group_serial = 0;        // tuning "group_serial" (rank 0 of a hakai_step_group): drain every rank's
                                 // phase before the next rank's (per-rank timings without the ranks
                                 // sharing the one GPU)
    hkc::DevBuf<double> d_pusai; // cal_Pusai_hexa table for the exact element kernel (192 doubles)
    int nmat = 0;
    long long elem_offset = 0;   // global id of local element 0
    // bc: the resolved tables of hakai_set_bc, sized for the model; `bc = {}` drops them
    struct BcTables {
        int n = 0;
        hkc::DevBuf<int> d_dof, d_grp;
        hkc::DevBuf<double> d_val;
        hkc::DevBuf<int> d_amp_n, d_amp_off;
        hkc::DevBuf<double> d_amp_t, d_amp_v;
        hkc::DevBuf<int> d_of_node;  // [nN] first resolved BC entry of each node (-1 none)
    } bc;
    int fuse_bc = 1;             // tuning "fuse_bc": the nodal kernel applies the BCs (one GPU)
    // state extras
    hkc::DevBuf<double> d_qbuf;  // the uploaded Q (sv.q == QSrc::Buf: the next nodal update reads it)
    std::vector<double> h_velo0;  // velo as uploaded / set by IC, valid until the first step
    double last_dt = 0.0;
    hkc::DevBuf<int> d_del_step; // [nEp+2] deletion step per element (0 = never), [nEp] dump slot,
                                 // [nEp+1] last step in which any element was deleted
    hkc::DevBuf<unsigned long long> d_negjac;
    hkc::DevBuf<int> d_poison;   // [2]: contact buffer overflow in this call (flag, step); see ElemArgs
    long long poison_step = -1;  // the step a contact overflow poisoned in the last failed call
    long long exchange_retries = 0;  // steps run again after a multi-GPU contact exchange overflow
    bool any_plastic = false;
    bool model_ok = false;
    bool state_ok = false;
    // host copies kept for setup work that needs the mesh (contact surfaces)
    std::vector<double> h_coord;  // 3nN
    std::vector<int> h_conn;      // 8nE, 0-based
    std::vector<int> h_mat;       // nE, 0-based
    std::vector<double> h_young;  // per material
    // external force (contact) -- null until contact is enabled; a non-owning view of
    // Contact::d_fext, set and cleared by the contact state
    double* d_fext = nullptr;
    hkc::Contact* contact = nullptr;
    // profiling
    bool prof = false;
    uint32_t prof_mask = 0;      // bit k: time kernel k (HAKAI_K_*)
    std::vector<hipEvent_t> ev_pool;
    std::vector<EventPair> ev_pending;
    double k_ms[HAKAI_K_COUNT] = {0, 0, 0, 0};
    long long k_n[HAKAI_K_COUNT] = {0, 0, 0, 0};
    // graph mode (hakai_step): `graph` steps (even) captured in one hipGraph per starting parity
    // (cur), plus a 2-step graph for the tail; the step number is read from a device counter
    // instead of kernel arguments. Slot [g][p]: g 0 = `graph` steps, 1 = 2 steps; p = parity.
    hkc::DevBuf<double> d_tstep;       // [2] counter slots (slot 1-cur: previous step's number)
    struct StepGraphs {
        const double* trd = nullptr;   // non-null while a step is captured: its counter slot
        hipGraphExec_t exec[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
        double dt[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        long long epoch[2][2] = {{-1, -1}, {-1, -1}};
        int len[2][2] = {{0, 0}, {0, 0}};
    } gr;
    long long epoch = 0;               // bumped by every call that may change buffers or settings
    long long tdev_next = -1;          // the step the device counter is valid for (-1: unknown)
    int graph = 16;                    // tuning "graph": steps per graph (even), 0 = no capture
    long long graph_steps = 0;         // steps run from graphs (tests, stats)
    hkc::Own own;                      // owner-computed assembly (hakai_own.hpp)
    // multi-GPU
    hkc::Comm* comm = nullptr;
    // history output (hakai_history_enable; hakai_history.hpp has the hooks)
    hkc::History* hist = nullptr;
    int hist_one_block = -1;           // tuning "history_one_block": -1 by size, 0 two launches, 1 one
    // element-set history (hakai_elem_history_enable / _probe; hakai_elem_history.hpp has the hooks)
    hkc::ElemHistory* ehist = nullptr;
    int ehist_one_block = -1;          // tuning "elem_history_one_block": -1 by size, 0 two launches, 1 one
    // stable-time-step diagnostic (hakai_stable_dt; hakai_stable_dt.hpp): its scratch, null until the
    // first call, and the Poisson ratios its material table needs next to h_young
    hkc::StableDt* sdt = nullptr;
    std::vector<double> h_poisson;     // per material
    // selective mass scaling (hakai_mass_scale; hakai_mass_scale.hpp): the elements' added mass and the
    // uploaded nodal mass, null until the first call (d_mass then holds the scaled mass)
    hkc::MassScale* msc = nullptr;
    // external loads and rigid walls (hakai_set_loads, hakai_set_walls; hakai_loads.hpp): null without
    // both. d_ftot [3nN] is the step's total external force, contact plus loads plus walls: a
    // non-owning view of Loads::ftot, set and cleared by that state
    hkc::Loads* loads = nullptr;
    double* d_ftot = nullptr;
};


namespace hkc {
// The external force every consumer of a step takes (nodal update, interface fix, history): the total
// of contact, loads and walls where loads or walls are set, else the contact force, else none.
inline const double* step_fext(const hakai_ctx* c) {
    return c->d_ftot ? c->d_ftot : (c->contact ? c->d_fext : nullptr);
}
// Grid of the persistent element kernel for this context (0: the one-batch-per-block kernel runs):
// only with >= pipe_min batches per block.
inline long long pipe_grid(const hakai_ctx* c) {
    const long long nb = c->nEp / hk::kEPB;
    const bool pipe = nb >= (long long)c->pipe_min * c->pipe_blocks && c->pipe_blocks > 0;
    return pipe ? (nb < c->pipe_blocks ? nb : c->pipe_blocks) : 0;
}
// Kernel arguments for the context's buffers with disp = d_u[cur] (hakai_capi.cpp): the element
// update without its owner-assembly part (own_elem_args), the nodal update without external force
// and fused BCs, the boundary conditions of step t.
hk::ElemArgs elem_args(const hakai_ctx* c, int cur);
hk::NodalArgs nodal_args(const hakai_ctx* c, double d_time);
hk::BCArgs bc_args(const hakai_ctx* c, double t, double d_time);
void prof_begin(hakai_ctx* c, int kernel, EventPair* p);
void prof_end(hakai_ctx* c, EventPair* p);
void comm_destroy(hakai_ctx* c);
int comm_reset(hakai_ctx* c);
void comm_pending_get(const hakai_ctx* c, bool* pending, int* par);
void comm_rollback(hakai_ctx* c, bool had_good, long long last_good, bool pending, int par);
// Multi-GPU hooks used by hakai_step (no-ops without a communicator).
int comm_pre_nodal(hakai_ctx* c);                    // save u_pre of interface nodes
// What the interface fix of a step read, for the history hook (hakai_history.hip hist_q_up forms the
// same Q at the nodes this rank owns): ran is false in a step without a fix (first step after a
// reset or an upload, an uploaded Q, no interface) -- the nodal kernel's own source is the Q then.
struct CommFix {
    bool ran = false;
    int n_up = 0, nslot = 0;
    const double* up_sendP = nullptr;  // [n_up][3], the parity the fix used
    const double* up_recvC = nullptr;  // [n_up][nslot][3]
};
int comm_post_nodal(hakai_ctx* c, double d_time, CommFix* fix = nullptr);  // wait exchange, fix interface nodes
int comm_post_element(hakai_ctx* c, long long step); // pack interface forces, start exchange
bool comm_is_local(const hakai_ctx* c);              // in-process group stepped in lockstep
const std::vector<int>* comm_dn_nodes(const hakai_ctx* c);  // nodes shared with rank-1 (or null)
const std::vector<int>* comm_up_nodes(const hakai_ctx* c);  // nodes shared with rank+1, in exchange order (or null)
bool comm_iface_set(const hakai_ctx* c);             // hakai_set_interface has run on this communicator
int comm_rank(const hakai_ctx* c);
int comm_size(const hakai_ctx* c);
// in-process group: dst + off[q] <- src[q] (bytes[q], 8-byte aligned), all ranks in one launch on
// c->stream (the caller orders it after the peers' producers)
constexpr int kMaxLocalGather = 64;
struct LocalGather {
    const char* src[kMaxLocalGather];
    long long bytes[kMaxLocalGather];
    long long off[kMaxLocalGather];
};
int gather_local(hakai_ctx* c, const LocalGather& g, int n, void* dst);
// RCCL only, ordered on c->stream: recv[q*bytes ..] = rank q's send; recv = MIN over ranks (uint64)
int comm_allgather_raw(hakai_ctx* c, const void* send, void* recv, size_t bytes);
int comm_allgatherv_raw(hakai_ctx* c, const void* send, void* recv, const size_t* bytes, const size_t* off);
int comm_allreduce_min_u64(hakai_ctx* c, const void* send, void* recv, size_t count);
bool comm_is_rccl(const hakai_ctx* c);
hakai_ctx* comm_peer_ctx(hakai_ctx* c, int q);                          // in-process group member q
// Contact (no-ops without hakai_set_contact): hakai_contact.hip; the multi-GPU phases, contact_step_b,
// contact_post_step and contact_exchange_retry: hakai_contact_xr.hip.
void contact_destroy(hakai_ctx* c);
int contact_state_reset(hakai_ctx* c, const double* velo0_host);
int contact_step(hakai_ctx* c, double t, double d_time);  // one GPU: contact force of step t -> d_fext
// The contact work of a step in phases (step_once's phase bits kPhaseA1 / A2 / A3): one GPU runs it
// all in part 1. Multi-GPU (hakai_set_contact_global): part 1 = deletions of the previous step,
// live lists, this rank's pair boxes; 2 = boxes combined, this rank's contact-zone nodes binned;
// 3 = every rank's binned nodes hashed, this rank's triangles searched, its events packed;
// contact_step_b = every rank's events gathered and summed. An in-process group runs each part on
// every rank before the next part on any (hakai_step_group).
int contact_phase(hakai_ctx* c, int part, double t, double d_time);
int contact_step_b(hakai_ctx* c);
bool contact_multi(const hakai_ctx* c);                   // multi-GPU contact (phase B runs)
int contact_post_step(hakai_ctx* c);                      // multi-GPU: pack this step's deletions
int contact_check(hakai_ctx* c);                          // buffer overflow check (syncs)
void contact_after_overflow(hakai_ctx* c, long long steps_since_reset);  // host state after a poisoned call
bool contact_exchange_retry(hakai_ctx* c);                // that call overflowed a multi-GPU exchange,
                                                          // now grown: the step may run again
void graph_invalidate(hakai_ctx* c);                      // drop captured step graphs (hakai_step.cpp)
void graph_free(hakai_ctx* c);
bool contact_graph_ok(const hakai_ctx* c, double t);       // step t's contact work can be captured
void contact_graph_advance(hakai_ctx* c, double t_last);   // host state after a cached graph's steps
int contact_tuning(hakai_ctx* c, const char* key, long long value);  // "contact_*" tuning keys
}  // namespace hkc
