// hakai_loads.hip -- external loads (hakai_set_loads, include/hakai_hip.h): concentrated nodal
// forces, gravity and follower face pressure, summed with the step's contact force into the total
// external force d_ftot that the nodal update, the interface fix and the history output consume.
//
// k_loads: ONE launch per step, one thread per node in 256-thread blocks over all nodes, no atomics.
// A node's sum has a fixed order (the header states it), so a thread GATHERS: its concentrated
// entries from a per-node list, the gravity entries, and its pressure contributions from a CSR node
// -> (entry, corner) that the host planner (hakai_loads_plan.cpp) built in ascending entry order. For
// a pressure contribution the thread loads the four corners of the face at the current configuration
// coord + u and evaluates only its own corner's F_a through hakai_loads_face.hpp -- g1, g2 and h are
// formed about four times per face over the launch, the price of a deterministic sum in one launch
// (small decks are launch-bound: a second launch would cost more than the arithmetic).
// The node's own operands (contact force, mass, list bounds) are loaded before the dependent gathers,
// as k_nodal does; which kinds of load exist is a launch-time constant (template parameters), so a
// node of a gravity-only model runs no list code and no runtime branch joins the loads; the time, the
// gravity entries and their amplitude tables are uniform over the launch.
// Rigid walls (hakai_set_walls) join the same sum in the same launch, after the pressure
// contributions: the fifth template parameter WL (0 no wall: the code of the four-flag kernel,
// 1 every wall takes every node, 2 a 32-bit membership mask per node). The loop over the walls is
// wave-uniform: the wall table and the walls' amplitude tables are read at uniform addresses
// (scalar loads), the wall's frame (two amplitude values, origin, velocity) is formed once per wave,
// and a lane's own work is the bit test, the gap and, under d > 0, hakai_walls_node.hpp's force. The
// node's coord, u_k, u_{k-1}, mass and mask are issued with its other operands, before the gathers.
// Loads and walls are independent parts of one device state that owns d_ftot.
// Compiled without contraction: the operation order of the header is the definition
// (tests/loads_ref.py and tests/walls_ref.py restate it, tests/test_gpu_loads.py and
// tests/test_gpu_walls.py compare bit for bit).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hakai_hip.h"
#include "hakai_history.hpp"
#include "hakai_internal.hpp"
#include "hakai_loads.hpp"
#include "hakai_loads_face.hpp"
#include "hakai_loads_plan.hpp"
#include "hakai_walls_node.hpp"
#include "hakai_walls_plan.hpp"

using hkc::fail;
using hkc::hip_fail;

namespace {

constexpr int kThreads = 256;

struct LoadArgs {
    const double* fc;      // the step's contact force [3nN], or null (+0.0)
    const double* mass;    // [nN]
    const double* coord;   // [3nN]
    const double* u;       // [3nN] the displacement the nodal update reads
    const int* conn;       // [8nE]
    const int* flag;       // [nE]
    double* ftot;          // [3nN]
    long long nN;
    double ct;             // t * d_time
    const double* t_rd;    // graph mode: ct = (*t_rd + 1.0) * dt, read on the device
    double dt;
    const int* amp_n;
    const int* amp_off;
    const double* amp_t;
    const double* amp_v;
    const int* cl_ptr;
    const int* cl_comp;
    const int* cl_amp;
    const double* cl_val;
    int n_grav;
    const double* g_acc;
    const int* g_amp;
    const int* pr_ptr;
    const int* pr_ent;
    const int* pr_elem;
    const int* pr_code;
    const int* pr_amp;
    const double* pr_val;
    // rigid walls (appended: the offsets of the fields above are those of the kernel without walls)
    const double* u_pre;   // [3nN] u_{k-1}, still intact before the nodal update
    double tau0, taum;     // (t - 1.0) * d_time, (t - 2.0) * d_time; graph mode: from *t_rd
    int n_wall;
    const double* w_tab;   // [kWallRow n_wall]
    const int* w_amp;      // [n_wall]
    const unsigned* w_mask;  // [nN], WL == 2
    const int* w_amp_n;
    const int* w_amp_off;
    const double* w_amp_t;
    const double* w_amp_v;
};

__device__ __forceinline__ double amp_of(const LoadArgs& a, int table, double ct) {
    if (table < 0) return 1.0;
    const int off = a.amp_off[table];
    return hk::loads_amp(a.amp_n[table], a.amp_t + off, a.amp_v + off, ct);
}

// FC: a contact force is added to; CL / GR / PR: concentrated, gravity, pressure entries exist;
// WL: walls exist (1: every wall takes every node, 2: per-node mask).
template <bool FC, bool CL, bool GR, bool PR, int WL>
__global__ __launch_bounds__(kThreads) void k_loads(LoadArgs a) {
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n >= a.nN) return;
    // the node's own operands, in flight together
    double f0 = FC ? a.fc[3 * n + 0] : 0.0;
    double f1 = FC ? a.fc[3 * n + 1] : 0.0;
    double f2 = FC ? a.fc[3 * n + 2] : 0.0;
    const double m = (GR || WL) ? a.mass[n] : 0.0;
    const int c0 = CL ? a.cl_ptr[n] : 0, c1 = CL ? a.cl_ptr[n + 1] : 0;
    const int p0 = PR ? a.pr_ptr[n] : 0, p1 = PR ? a.pr_ptr[n + 1] : 0;
    double xc[3] = {0.0, 0.0, 0.0}, uk[3] = {0.0, 0.0, 0.0}, um[3] = {0.0, 0.0, 0.0};
    unsigned wmask = 0xffffffffu;
    if (WL) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xc[c] = a.coord[3 * n + c];
            uk[c] = a.u[3 * n + c];
            um[c] = a.u_pre[3 * n + c];
        }
        if (WL == 2) wmask = a.w_mask[n];
    }
    const double ct = a.t_rd ? (*a.t_rd + 1.0) * a.dt : a.ct;  // t * d_time, as on the host
    if (CL) {
        for (int j = c0; j < c1; ++j) {
            const double v = a.cl_val[j] * amp_of(a, a.cl_amp[j], ct);
            const int cc = a.cl_comp[j];
            f0 = cc == 0 ? f0 + v : f0;
            f1 = cc == 1 ? f1 + v : f1;
            f2 = cc == 2 ? f2 + v : f2;
        }
    }
    if (GR) {
        for (int g = 0; g < a.n_grav; ++g) {  // uniform: scalar loads
            const double amp = amp_of(a, a.g_amp[g], ct);
            f0 = f0 + m * (a.g_acc[3 * g + 0] * amp);
            f1 = f1 + m * (a.g_acc[3 * g + 1] * amp);
            f2 = f2 + m * (a.g_acc[3 * g + 2] * amp);
        }
    }
    if (PR) {
        for (int j = p0; j < p1; ++j) {
            const int ent = a.pr_ent[j];
            const int k = ent >> 2, corner = ent & 3;
            const long long e = a.pr_elem[k];
            const unsigned code = (unsigned)a.pr_code[k];
            const int active = a.flag[e];
            const double pa = a.pr_val[k] * amp_of(a, a.pr_amp[k], ct);
            double x[4][3];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long nq = a.conn[8 * e + hk::loads_code_node(code, q)];
#pragma unroll
                for (int c = 0; c < 3; ++c) x[q][c] = a.coord[3 * nq + c] + a.u[3 * nq + c];
            }
            double F[3];
            hk::loads_face_corner(x, corner, pa, F);
            if (active == 1) {  // a deleted element's face stops loading
                f0 = f0 + F[0];
                f1 = f1 + F[1];
                f2 = f2 + F[2];
            }
        }
    }
    if (WL) {
        const double tau0 = a.t_rd ? (*a.t_rd) * a.dt : a.tau0;          // (t - 1.0) * d_time
        const double taum = a.t_rd ? (*a.t_rd - 1.0) * a.dt : a.taum;    // (t - 2.0) * d_time
        for (int w = 0; w < a.n_wall; ++w) {  // uniform: scalar loads, one frame per wave
            const double* row = a.w_tab + hk::kWallRow * w;
            const int table = a.w_amp[w];
            double s0 = 1.0, sm = 1.0;
            if (table >= 0) {
                const int off = a.w_amp_off[table], nr = a.w_amp_n[table];
                s0 = hk::loads_amp(nr, a.w_amp_t + off, a.w_amp_v + off, tau0);
                sm = hk::loads_amp(nr, a.w_amp_t + off, a.w_amp_v + off, taum);
            }
            double o[3], vw[3];
            hk::walls_frame(row + 3, row + 6, s0, sm, a.dt, o, vw);
            const double d = -hk::walls_gap(xc, uk, o, row);
            if (((wmask >> w) & 1u) && d > 0.0) {
                double F[3];
                hk::walls_force(d, uk, um, m, a.dt, vw, row, row[9], row[10], row[11], row[12], F);
                f0 = f0 + F[0];
                f1 = f1 + F[1];
                f2 = f2 + F[2];
            }
        }
    }
    a.ftot[3 * n + 0] = f0;
    a.ftot[3 * n + 1] = f1;
    a.ftot[3 * n + 2] = f2;
}

template <bool FC, bool CL, bool GR, bool PR>
void launch_wl(const LoadArgs& a, int wl, unsigned grid, hipStream_t s) {
    if (wl == 2)
        hipLaunchKernelGGL((k_loads<FC, CL, GR, PR, 2>), dim3(grid), dim3(kThreads), 0, s, a);
    else if (wl == 1)
        hipLaunchKernelGGL((k_loads<FC, CL, GR, PR, 1>), dim3(grid), dim3(kThreads), 0, s, a);
    else
        hipLaunchKernelGGL((k_loads<FC, CL, GR, PR, 0>), dim3(grid), dim3(kThreads), 0, s, a);
}
template <bool FC, bool CL, bool GR>
void launch_pr(const LoadArgs& a, bool pr, int wl, unsigned grid, hipStream_t s) {
    if (pr)
        launch_wl<FC, CL, GR, true>(a, wl, grid, s);
    else
        launch_wl<FC, CL, GR, false>(a, wl, grid, s);
}
template <bool FC, bool CL>
void launch_gr(const LoadArgs& a, bool gr, bool pr, int wl, unsigned grid, hipStream_t s) {
    if (gr)
        launch_pr<FC, CL, true>(a, pr, wl, grid, s);
    else
        launch_pr<FC, CL, false>(a, pr, wl, grid, s);
}
template <bool FC>
void launch_cl(const LoadArgs& a, bool cl, bool gr, bool pr, int wl, unsigned grid, hipStream_t s) {
    if (cl)
        launch_gr<FC, true>(a, gr, pr, wl, grid, s);
    else
        launch_gr<FC, false>(a, gr, pr, wl, grid, s);
}

// A planned array on its way to the device; an empty one allocates nothing and stays a null pointer.
template <class T>
hipError_t upload(hkc::DevBuf<T>& d, const std::vector<T>& h, hipStream_t s) {
    return h.empty() ? hipSuccess : d.upload(h, s);
}

}  // namespace

namespace hkc {

// Device state of the external force: the loads' plan (hakai_loads_plan.hpp), the walls' plan
// (hakai_walls_plan.hpp) -- either may be absent, not both -- and the total external force of the step.
struct Loads {
    DevBuf<double> ftot;                 // [3nN], c->d_ftot
    struct LoadBufs {                    // hakai_set_loads' plan (LoadArgs has the fields' meaning)
        DevBuf<int> amp_n, amp_off;
        DevBuf<double> amp_t, amp_v;
        DevBuf<int> cl_ptr, cl_comp, cl_amp;
        DevBuf<double> cl_val, g_acc;
        DevBuf<int> g_amp, pr_ptr, pr_ent, pr_elem, pr_code, pr_amp;
        DevBuf<double> pr_val;
    } lb;
    struct WallBufs {                    // hakai_set_walls' plan
        DevBuf<int> amp_n, amp_off;
        DevBuf<double> amp_t, amp_v, tab;
        DevBuf<int> amp;
        DevBuf<unsigned> mask;
    } wb;
    int n_grav = 0, n_wall = 0;
    bool cl = false, gr = false, pr = false;
    int wl = 0;                          // 0 no wall, 1 every wall takes every node, 2 mask
    bool has_loads() const { return cl || gr || pr; }
};

void loads_destroy(hakai_ctx* c) {
    if (!c || !c->loads) return;
    (void)hipSetDevice(c->device);
    delete c->loads;
    c->loads = nullptr;
    c->d_ftot = nullptr;  // (a view of the state above)
}

// The state to add a part to: the context's, or a new one with its d_ftot.
static int loads_state(hakai_ctx* c) {
    if (c->loads) return 0;
    std::unique_ptr<Loads> L(new Loads());
    HIPCHK(L->ftot.alloc(3 * (size_t)c->nN));
    c->loads = L.release();
    c->d_ftot = c->loads->ftot;
    return 0;
}

// with_loads / with_walls: the parts of the sum to form (a step: both; the probes: one each)
static int loads_launch(hakai_ctx* c, double t, double d_time, const double* fc, const double* t_rd, hipStream_t s,
                        bool with_loads, bool with_walls) {
    const Loads* L = c->loads;
    LoadArgs a;
    std::memset(&a, 0, sizeof a);
    const Loads::LoadBufs& b = L->lb;
    a.amp_n = b.amp_n, a.amp_off = b.amp_off, a.amp_t = b.amp_t, a.amp_v = b.amp_v;
    a.cl_ptr = b.cl_ptr, a.cl_comp = b.cl_comp, a.cl_amp = b.cl_amp, a.cl_val = b.cl_val;
    a.g_acc = b.g_acc, a.g_amp = b.g_amp, a.n_grav = L->n_grav;
    a.pr_ptr = b.pr_ptr, a.pr_ent = b.pr_ent, a.pr_elem = b.pr_elem, a.pr_code = b.pr_code, a.pr_amp = b.pr_amp,
    a.pr_val = b.pr_val;
    const Loads::WallBufs& w = L->wb;
    a.w_amp_n = w.amp_n, a.w_amp_off = w.amp_off, a.w_amp_t = w.amp_t, a.w_amp_v = w.amp_v;
    a.w_tab = w.tab, a.w_amp = w.amp, a.w_mask = w.mask, a.n_wall = L->n_wall;
    a.fc = fc;
    a.mass = c->d_mass;
    a.coord = c->d_coord;
    a.u = c->d_u[c->sv.cur];
    a.u_pre = c->d_u[1 - c->sv.cur];
    a.conn = c->d_conn;
    a.flag = c->d_flag;
    a.ftot = c->d_ftot;
    a.nN = c->nN;
    a.ct = t * d_time;
    a.tau0 = (t - 1.0) * d_time;
    a.taum = (t - 2.0) * d_time;
    a.t_rd = t_rd;
    a.dt = d_time;
    const unsigned grid = (unsigned)((c->nN + kThreads - 1) / kThreads);
    const bool cl = with_loads && L->cl, gr = with_loads && L->gr, pr = with_loads && L->pr;
    const int wl = with_walls ? L->wl : 0;
    if (fc)
        launch_cl<true>(a, cl, gr, pr, wl, grid, s);
    else
        launch_cl<false>(a, cl, gr, pr, wl, grid, s);
    HIPCHK(hipGetLastError());
    return 0;
}

int loads_step(hakai_ctx* c, double t, double d_time, const double* fc) {
    if (!c->loads) return 0;
    return loads_launch(c, t, d_time, fc, c->gr.trd, c->stream, true, true);
}

// A probe: one part of the sum alone, at the current state. d_ftot is rewritten whole by every step
// before anything reads it: the probe may use it.
static int loads_probe(hakai_ctx* c, double t, double d_time, double* f, bool walls, const char* what) {
    if (!c || !f) return fail(HAKAI_ERR_ARG, "null");
    if (!c->state_ok) return fail(HAKAI_ERR_STATE, "%s without state", what);
    const size_t fn = 3 * (size_t)c->nN;
    HIPCHK(hipSetDevice(c->device));
    if (!c->loads || (walls ? c->loads->wl == 0 : !c->loads->has_loads())) {
        for (size_t i = 0; i < fn; ++i) f[i] = 0.0;
        return 0;
    }
    if (int r = loads_launch(c, t, d_time, nullptr, nullptr, c->stream, !walls, walls)) return r;
    HIPCHK(hipMemcpyAsync(f, c->d_ftot, fn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace hkc

extern "C" {

int hakai_clear_loads(hakai_ctx* c) {
    if (c) hkc::graph_invalidate(c);  // the launch sequence changes
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "clear_loads before upload_model");
    if (!c->loads || !c->loads->has_loads()) return 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    hkc::Loads* L = c->loads;
    if (L->wl == 0) {
        hkc::loads_destroy(c);
    } else {  // the walls stay in force
        L->lb = hkc::Loads::LoadBufs();
        L->cl = L->gr = L->pr = false;
        L->n_grav = 0;
    }
    return hkc::history_restart(c);  // W_ext changes its meaning
}

int hakai_set_loads(hakai_ctx* c, const hakai_loads_t* in) {
    if (c) hkc::graph_invalidate(c);  // the launch sequence changes
    if (!c || !in) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "set_loads before upload_model");
    hk::LoadsPlan P;
    std::string err;
    if (hk::loads_plan(*in, c->nN, c->nE, c->h_conn.data(), P, err)) return fail(HAKAI_ERR_ARG, "%s", err.c_str());
    if (c->comm && in->n_press > 0)
        return fail(HAKAI_ERR_STATE, "set_loads: face pressure on a context with a communicator is not supported "
                    "(a face across a cut needs nodes the rank does not hold)");
    if (in->n_cload == 0 && in->n_grav == 0 && in->n_press == 0) return hakai_clear_loads(c);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(hipStreamSynchronize(s));
    hkc::Loads::LoadBufs b;
    HIPCHK(upload(b.amp_n, P.amp_n, s));
    HIPCHK(upload(b.amp_off, P.amp_off, s));
    HIPCHK(upload(b.amp_t, P.amp_t, s));
    HIPCHK(upload(b.amp_v, P.amp_v, s));
    HIPCHK(upload(b.cl_ptr, P.cl_ptr, s));
    HIPCHK(upload(b.cl_comp, P.cl_comp, s));
    HIPCHK(upload(b.cl_amp, P.cl_amp, s));
    HIPCHK(upload(b.cl_val, P.cl_val, s));
    HIPCHK(upload(b.g_acc, P.g_acc, s));
    HIPCHK(upload(b.g_amp, P.g_amp, s));
    HIPCHK(upload(b.pr_ptr, P.pr_ptr, s));
    HIPCHK(upload(b.pr_ent, P.pr_ent, s));
    HIPCHK(upload(b.pr_elem, P.pr_elem, s));
    HIPCHK(upload(b.pr_code, P.pr_code, s));
    HIPCHK(upload(b.pr_amp, P.pr_amp, s));
    HIPCHK(upload(b.pr_val, P.pr_val, s));
    HIPCHK(hipStreamSynchronize(s));  // the plan's vectors go out of scope
    if (int r = hkc::loads_state(c)) return r;
    hkc::Loads* L = c->loads;
    L->lb = std::move(b);  // (the previous plan's arrays are freed here)
    L->n_grav = (int)P.g_amp.size();
    L->cl = !P.cl_ptr.empty();
    L->gr = L->n_grav > 0;
    L->pr = !P.pr_ptr.empty();
    return hkc::history_restart(c);  // W_ext changes its meaning
}

int hakai_load_force(hakai_ctx* c, double t, double d_time, double* f) {
    return hkc::loads_probe(c, t, d_time, f, false, "load_force");
}

int hakai_clear_walls(hakai_ctx* c) {
    if (c) hkc::graph_invalidate(c);  // the launch sequence changes
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "clear_walls before upload_model");
    if (!c->loads || c->loads->wl == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    hkc::Loads* L = c->loads;
    if (!L->has_loads()) {
        hkc::loads_destroy(c);
    } else {  // the loads stay in force
        L->wb = hkc::Loads::WallBufs();
        L->wl = 0;
        L->n_wall = 0;
    }
    return hkc::history_restart(c);  // W_ext changes its meaning
}

int hakai_set_walls(hakai_ctx* c, const hakai_walls_t* in) {
    if (c) hkc::graph_invalidate(c);  // the launch sequence changes
    if (!c || !in) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "set_walls before upload_model");
    hk::WallsPlan P;
    std::string err;
    if (hk::walls_plan(*in, c->nN, P, err)) return fail(HAKAI_ERR_ARG, "%s", err.c_str());
    if (P.n_wall == 0) return hakai_clear_walls(c);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(hipStreamSynchronize(s));
    hkc::Loads::WallBufs b;
    HIPCHK(upload(b.amp_n, P.amp_n, s));
    HIPCHK(upload(b.amp_off, P.amp_off, s));
    HIPCHK(upload(b.amp_t, P.amp_t, s));
    HIPCHK(upload(b.amp_v, P.amp_v, s));
    HIPCHK(upload(b.tab, P.tab, s));
    HIPCHK(upload(b.amp, P.amp, s));
    HIPCHK(upload(b.mask, P.mask, s));
    HIPCHK(hipStreamSynchronize(s));  // the plan's vectors go out of scope
    if (int r = hkc::loads_state(c)) return r;
    hkc::Loads* L = c->loads;
    L->wb = std::move(b);  // (the previous plan's arrays are freed here)
    L->n_wall = P.n_wall;
    L->wl = P.mask.empty() ? 1 : 2;
    return hkc::history_restart(c);  // W_ext changes its meaning
}

int hakai_wall_force(hakai_ctx* c, double t, double d_time, double* f) {
    return hkc::loads_probe(c, t, d_time, f, true, "wall_force");
}

}  // extern "C"
