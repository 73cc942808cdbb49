// hakai_capi.cpp -- C ABI of libhakai_hip.so (declared in include/hakai_hip.h).
//
// Owns the persistent device context: model, Gauss-point state in SoA, ping-pong displacement
// buffers, the node->element incidence CSR used for the deterministic force gather, BC tables,
// deletion log and per-kernel HIP-event timers. One HIP stream per context.
//
// Where the code is: this file has the context's creation and destruction, the model, BC and state
// uploads and downloads, profiling, the tuning and stat keys (owner keys: hakai_own.cpp, contact
// keys: hakai_contact.hip), the deletion log, negative Jacobians, node averages, the stateless
// drop-ins and the kernel-argument builders. hakai_step.cpp is the step driver (one step, graph
// capture and replay, the overflow rollback, hakai_step and hakai_step_group); hakai_step_view.hpp
// the host's view of the stepping state, whose member functions alone change it; hakai_own.cpp the
// run time of owner-computed assembly (hkc::Own); hakai_devmem.hpp the HIP error check and
// hkc::DevBuf, the owner of every device array: the context's are its members (hakai_internal.hpp) and
// free themselves with it, a function's temporaries are locals.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hakai_hip.h"
#include "hakai_conn_plan.hpp"
#include "hakai_elem_history.hpp"
#include "hakai_history.hpp"
#include "hakai_internal.hpp"
#include "hakai_kernels.hpp"
#include "hakai_loads.hpp"
#include "hakai_mass_scale.hpp"
#include "hakai_stable_dt.hpp"

using hk::DevMat;

namespace {
thread_local std::string g_err;
}

namespace hkc {

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(HAKAI_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace hkc

using hkc::DevBuf;
using hkc::fail;
using hkc::hip_fail;
using hkc::QSrc;

namespace hkc {

// Releases the previous mesh's arrays before hakai_upload_model allocates the next one's, so a
// re-upload's peak memory is one mesh. Every array frees itself with the context: one missing from
// this list is held until the next upload overwrites it or the context goes, never leaked.
static void free_model(hakai_ctx* c) {
    contact_destroy(c);
    loads_destroy(c);  // sized and validated for the previous mesh
    for (DevBuf<double>* b : {&c->d_coord, &c->d_u[0], &c->d_u[1], &c->d_mass, &c->d_stress, &c->d_strain, &c->d_eqps,
                              &c->d_yield, &c->d_triax, &c->d_fe, &c->d_qbuf})
        b->free();
    for (DevBuf<int>* b : {&c->d_conn, &c->d_flag, &c->d_mat, &c->d_inc_ptr, &c->d_inc, &c->d_inc_row, &c->d_inc8,
                           &c->d_del_step})
        b->free();
    c->d_mats.free();
    c->d_conn_rec.free();
    c->conn_P = 0;
    own_free(c);
    c->model_ok = false;
    c->state_ok = false;
}

// Material constants exactly as hakai() derives them (v2/HAKAI_j.jl:143-160) and readInpFile
// builds Hd (v2/readInpFile_j.jl:763-768).
int build_devmat(const hakai_material_t& in, DevMat& o) {
    std::memset(&o, 0, sizeof o);
    const double young = in.young, poisson = in.poisson;
    const double d1 = (1.0 - poisson), d2 = poisson, d3 = (1.0 - 2.0 * poisson) / 2.0;
    const double cc = young / (1.0 + poisson) / (1.0 - 2.0 * poisson);
    o.Dn = cc * d1;
    o.Do = cc * d2;
    o.Ds = cc * d3;
    o.G = young / 2. / (1.0 + poisson);
    o.density = in.density;
    if (in.n_plastic < 0 || in.n_plastic > hk::kMaxPlastic)
        return fail(HAKAI_ERR_ARG, "material: %d plastic rows (max %d)", in.n_plastic, hk::kMaxPlastic);
    if (in.n_ductile < 0 || in.n_ductile > hk::kMaxDuctile)
        return fail(HAKAI_ERR_ARG, "material: %d ductile rows (max %d)", in.n_ductile, hk::kMaxDuctile);
    if (in.n_plastic == 1)
        return fail(HAKAI_ERR_MODEL,
                    "material: a single *Plastic row gives an empty Hd; the reference raises BoundsError "
                    "(v2/HAKAI_j.jl:1267)");
    o.npp = in.n_plastic;
    o.nd = in.n_ductile;
    o.yield0 = in.n_plastic > 0 ? in.plastic[0] : 0.0;
    for (int r = 0; r < in.n_plastic; ++r) o.pl_eps[r] = in.plastic[2 * r + 1];
    for (int r = 0; r + 1 < in.n_plastic; ++r)
        o.Hd[r] = (in.plastic[2 * (r + 1)] - in.plastic[2 * r]) / (in.plastic[2 * (r + 1) + 1] - in.plastic[2 * r + 1]);
    for (int r = 0; r < in.n_ductile; ++r) {
        o.du_eps[r] = in.ductile[3 * r + 0];
        o.du_tri[r] = in.ductile[3 * r + 1];
    }
    // ductile_fr returns a table value or a linear interpolation between two neighbouring ones,
    // i.e. at least the smallest fracture strain less a few rounding errors of its terms: an element
    // average below min - (|max| + |min|) * 2^-40 cannot reach it, and the kernels skip the table
    // search (the same deletion decisions, tests/test_gpu_exact.py, test_gpu_fullsize.py)
    double lo = 0.0, hi = 0.0;
    for (int r = 0; r < in.n_ductile; ++r) {
        lo = r == 0 ? o.du_eps[r] : std::min(lo, o.du_eps[r]);
        hi = r == 0 ? o.du_eps[r] : std::max(hi, o.du_eps[r]);
    }
    o.du_floor = in.n_ductile > 0 ? lo - (std::fabs(hi) + std::fabs(lo)) * 0x1p-40 : 0.0;
    if (!(o.du_floor == o.du_floor)) o.du_floor = -HUGE_VAL;  // (a NaN table: never skip)
    // an element average of eight values below du_skip (rounded sums: at most 8 ulps above their
    // bound) stays below du_floor: a wave whose Gauss points all lie below it needs no averages
    o.du_skip = o.du_floor > 0.0 ? o.du_floor - o.du_floor * 0x1p-40 : -HUGE_VAL;
    return 0;
}

// cal_Pusai_hexa (v2/HAKAI_j.jl:1895-1943): dN_i/dxi at the 8 Gauss points, out[24k + 8r + i],
// with the reference's expression order (this file is compiled without contraction).
void pusai_table(double out[192]) {
    static const double delta[8][3] = {{-1.0, -1.0, -1.0}, {1.0, -1.0, -1.0}, {1.0, 1.0, -1.0}, {-1.0, 1.0, -1.0},
                                       {-1.0, -1.0, 1.0},  {1.0, -1.0, 1.0},  {1.0, 1.0, 1.0},  {-1.0, 1.0, 1.0}};
    const double g = 1.0 / std::sqrt(3.0);
    for (int k = 0; k < 8; ++k) {  // gc order :1913-1920: k bits = (xi, eta, zeta) signs
        const double gzai = (k & 4) ? g : -g, eta = (k & 2) ? g : -g, tueta = (k & 1) ? g : -g;
        for (int i = 0; i < 8; ++i) {
            out[24 * k + i] = 1.0 / 8.0 * delta[i][0] * (1.0 + eta * delta[i][1]) * (1.0 + tueta * delta[i][2]);
            out[24 * k + 8 + i] = 1.0 / 8.0 * delta[i][1] * (1.0 + gzai * delta[i][0]) * (1.0 + tueta * delta[i][2]);
            out[24 * k + 16 + i] = 1.0 / 8.0 * delta[i][2] * (1.0 + gzai * delta[i][0]) * (1.0 + eta * delta[i][1]);
        }
    }
}

hipStream_t ctx_stream(hakai_ctx* c) { return c->stream; }
int ctx_device(hakai_ctx* c) { return c->device; }

}  // namespace hkc

// ---------------------------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------------------------
static void prof_harvest(hakai_ctx* c) {
    if (c->ev_pending.empty()) return;
    (void)hipEventSynchronize(c->ev_pending.back().b);
    for (auto& p : c->ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->k_ms[p.kernel] += ms;
            c->k_n[p.kernel] += 1;
        }
        c->ev_pool.push_back(p.a);
        c->ev_pool.push_back(p.b);
    }
    c->ev_pending.clear();
}

static hipEvent_t prof_event(hakai_ctx* c) {
    if (c->ev_pool.empty()) {
        if (c->ev_pending.size() >= 2048) prof_harvest(c);
        if (c->ev_pool.empty()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            return e;
        }
    }
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
}

namespace hkc {
void prof_begin(hakai_ctx* c, int kernel, EventPair* p) {
    p->kernel = -1;
    if (!c->prof || !((c->prof_mask >> kernel) & 1u)) return;
    p->kernel = kernel;
    p->a = prof_event(c);
    p->b = prof_event(c);
    (void)hipEventRecord(p->a, c->stream);
}
void prof_end(hakai_ctx* c, EventPair* p) {
    if (!c->prof || p->kernel < 0) return;
    (void)hipEventRecord(p->b, c->stream);
    c->ev_pending.push_back(*p);
}
}  // namespace hkc


namespace hkc {

// Kernel arguments of the element update with disp = d_u[cur].
hk::ElemArgs elem_args(const hakai_ctx* c, int cur) {
    hk::ElemArgs ea;
    std::memset(&ea, 0, sizeof ea);
    ea.coord = c->d_coord;
    ea.u = c->d_u[cur];
    ea.u_pre = c->d_u[1 - cur];
    ea.conn = c->d_conn;
    ea.flag = c->d_flag;
    ea.mat = c->d_mat;
    // one material: every entry of d_mat is 0 (hakai_upload_model), so the kernels read d_mat[0]
    // for every element instead of streaming the array
    ea.mat_stride = c->nmat == 1 ? 0u : 4u;
    ea.mats = c->d_mats;
    ea.stress = c->d_stress;
    ea.strain = c->d_strain;
    for (int q = 0; q < 6; ++q) {
        ea.sc[q] = c->d_stress + q * c->ld;
        ea.ec[q] = c->d_strain + q * c->ld;
    }
    ea.eqps = c->d_eqps;
    ea.yield = c->d_yield;
    ea.triax = c->d_triax;
    ea.fe = c->d_fe;
    ea.vol = nullptr;
    ea.nE = c->nE;
    ea.nEp = c->nEp;
    ea.ld = c->ld;
    ea.del_step = c->d_del_step;
    ea.step_i = 0;
    ea.any_plastic = c->any_plastic ? 1 : 0;
    // small meshes take the one-batch-per-block kernel
    ea.pipe_blocks = pipe_grid(c) > 0 ? c->pipe_blocks : 0;
    ea.gp_nt = c->gp_nt;
    ea.nmat = c->nmat;
    ea.exact = c->elem_exact;
    ea.pusai = c->d_pusai;
    ea.poison = c->d_poison;
    return ea;
}

// Kernel arguments of the nodal update: Q from the uploaded-Q buffer, the previous element step's
// owner-computed sums, or the fe gather (sv.q); the caller adds the external force and fused BCs.
hk::NodalArgs nodal_args(const hakai_ctx* c, double d_time) {
    hk::NodalArgs na;
    na.u = c->d_u[c->sv.cur];
    na.u_pre_out = c->d_u[1 - c->sv.cur];
    na.mass = c->d_mass;
    na.inc_ptr = c->d_inc_ptr;
    na.inc = c->d_inc;
    na.inc8 = c->d_inc8;
    na.fe = c->d_fe;
    na.qbuf = c->sv.q == QSrc::Buf ? c->d_qbuf : nullptr;
    na.fext = nullptr;
    na.nN = c->nN;
    na.dt = d_time;
    na.bc_of_node = nullptr;
    const OwnSums o = c->sv.q == QSrc::Own ? own_sums(c) : OwnSums{nullptr, nullptr, nullptr, nullptr};
    na.own_q = o.q;
    na.own_rp = o.rp;
    na.own_rows = o.rows;
    na.own_ridx = o.ridx;
    na.poison = c->d_poison;
    return na;
}

// Kernel arguments of the boundary conditions of step t, written into disp_new.
hk::BCArgs bc_args(const hakai_ctx* c, double t, double d_time) {
    hk::BCArgs ba;
    ba.dof = c->bc.d_dof;
    ba.grp = c->bc.d_grp;
    ba.val = c->bc.d_val;
    ba.n = c->bc.n;
    ba.amp_n = c->bc.d_amp_n;
    ba.amp_off = c->bc.d_amp_off;
    ba.amp_t = c->bc.d_amp_t;
    ba.amp_v = c->bc.d_amp_v;
    ba.out = c->d_u[1 - c->sv.cur];
    ba.ct = t * d_time;
    ba.t_rd = c->gr.trd;
    ba.dt = d_time;
    ba.poison = c->d_poison;
    return ba;
}

}  // namespace hkc

// Element forces [nEp][8][3] <-> the reference's Qe (24 x nE): the same layout.
static int fe_download_qe(hakai_ctx* c, double* Qe) {
    HIPCHK(hipMemcpyAsync(Qe, c->d_fe, 24 * (size_t)c->nE * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

static int fe_upload_qe(hakai_ctx* c, const double* Qe) {
    HIPCHK(hipMemcpyAsync(c->d_fe, Qe, 24 * (size_t)c->nE * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// Incidence tables (CSR and padded) as force row bases 24e + 3k; padding -> the zero base 24nEp.
static int fe_upload_incidence(hakai_ctx* c) {
    std::vector<int> inc(c->h_inc0.size());
    for (size_t j = 0; j < inc.size(); ++j) inc[j] = 24 * (c->h_inc0[j] >> 3) + 3 * (c->h_inc0[j] & 7);
    if (!inc.empty())
        HIPCHK(hipMemcpyAsync(c->d_inc, inc.data(), inc.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (c->d_inc8) {
        std::vector<int> inc8(8 * (size_t)c->nN, (int)(24 * c->nEp));
        for (long long n = 0; n < c->nN; ++n)
            for (int j = c->h_ptr[n]; j < c->h_ptr[n + 1]; ++j) inc8[8 * n + (j - c->h_ptr[n])] = inc[j];
        HIPCHK(hipMemcpyAsync(c->d_inc8, inc8.data(), inc8.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------
extern "C" {

int hakai_abi_version(void) { return HAKAI_ABI_VERSION; }
const char* hakai_last_error(void) { return g_err.c_str(); }

int hakai_device_count(int* n) {
    if (!n) return fail(HAKAI_ERR_ARG, "null");
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) cnt = 0;
    *n = cnt;
    return 0;
}

int hakai_create(hakai_ctx** out, int device) {
    if (!out) return fail(HAKAI_ERR_ARG, "null ctx pointer");
    *out = nullptr;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
        return fail(HAKAI_ERR_DEVICE, "no HIP device visible: the HAKAI MI355X path has no CPU fallback");
    if (device < 0 || device >= cnt) return fail(HAKAI_ERR_ARG, "device %d out of range (%d visible)", device, cnt);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(HAKAI_ERR_DEVICE, "device %d is %s; libhakai_hip is built for gfx950 only", device,
                    prop.gcnArchName);
    // (until the function succeeds: a return on any path below destroys what exists so far)
    struct Drop {
        void operator()(hakai_ctx* p) const {
            if (p->stream) (void)hipStreamDestroy(p->stream);
            delete p;
        }
    };
    std::unique_ptr<hakai_ctx, Drop> c(new hakai_ctx());
    c->device = device;
    if (const char* v = std::getenv("HAKAI_PIPE_BLOCKS")) c->pipe_blocks = std::atoi(v);
    // HAKAI_GRAPH=n: steps per captured graph (0 = stream mode). rocprofv3 --kernel-trace crashes
    // the host process on any hipGraph launch with this ROCm (tools/graph_probe.hip alone
    // reproduces it), so the profiling scripts run with HAKAI_GRAPH=0.
    if (const char* v = std::getenv("HAKAI_GRAPH")) {
        const int g = std::atoi(v);
        c->graph = (g >= 0 && g <= 1024 && !(g & 1)) ? g : 0;
    }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
    if (c->d_negjac.alloc(1) != hipSuccess || c->d_pusai.alloc(192) != hipSuccess ||
        c->d_poison.alloc(2) != hipSuccess || hipMemset(c->d_poison, 0, 2 * sizeof(int)) != hipSuccess)
        return fail(HAKAI_ERR_DEVICE, "hipMalloc for context bookkeeping failed");
    {
        double pus[192];
        hkc::pusai_table(pus);
        // the reference-order element step forms each P2 product once per partner pair and takes
        // the partner's as its exact negation (elem_step_exact): the table must be odd in each sign
        bool odd = true;
        for (int k = 0; k < 8; ++k)
            for (int i = 0; i < 8; ++i) {
                const double* p = pus + 24 * k;
                odd = odd && p[i] == -p[i ^ 1] && p[8 + i] == -p[8 + (i ^ 3)] && p[16 + i] == -p[16 + (i ^ 4)];
            }
        e = odd ? hipMemcpy(c->d_pusai, pus, sizeof pus, hipMemcpyHostToDevice) : hipErrorInvalidValue;
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy (Pusai table)");
    }
    if (const char* v = std::getenv("HAKAI_ELEM_EXACT")) c->elem_exact = std::atoi(v) ? 1 : 0;
    if (const char* v = std::getenv("HAKAI_OWN_ASSEMBLY")) c->own.assembly = std::atoi(v) ? 1 : 0;
    *out = c.release();
    return 0;
}

int hakai_destroy(hakai_ctx* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    prof_harvest(c);
    hkc::graph_free(c);
    hkc::history_destroy(c);
    hkc::elem_history_destroy(c);
    hkc::stable_dt_destroy(c);
    hkc::mass_scale_destroy(c);
    hkc::comm_destroy(c);
    hkc::free_model(c);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    delete c;  // (the context's remaining arrays free themselves)
    return 0;
}

int hakai_upload_model(hakai_ctx* c, int64_t nNode, const double* coordmat, int64_t nElement,
                       const int64_t* elementmat, const int64_t* element_material, int32_t nMat,
                       const hakai_material_t* mats, const double* diag_M) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c) return fail(HAKAI_ERR_ARG, "null ctx");
    if (nNode <= 0 || nElement < 0 || !coordmat || (nElement > 0 && (!elementmat || !element_material)) || nMat <= 0 ||
        !mats || !diag_M)
        return fail(HAKAI_ERR_ARG, "upload_model: bad arguments");
    if (26 * (nElement + 32) + 8 >= (int64_t)INT32_MAX || nNode >= (int64_t)INT32_MAX)
        return fail(HAKAI_ERR_ARG, "upload_model: mesh too large for int32 indexing on one rank");
    // the element kernel addresses its arrays with a 32-bit byte offset per lane (the element
    // forces, 192 B per element, are the largest): at most ~22 M hex per context; larger meshes
    // are split over ranks (hakai_comm_init / hakai_comm_init_local, also on one GPU)
    if (192 * (nElement + 32) >= (int64_t)1 << 32)
        return fail(HAKAI_ERR_ARG, "upload_model: %lld elements exceed one context's 32-bit element-kernel offsets "
                    "(max %lld); split the mesh over ranks", (long long)nElement, (long long)(((int64_t)1 << 32) / 192 - 32));
    // (node gathers: 24 B per node, load_node / load_node_raw form 24u * n)
    if (24 * (nNode + 1) >= (int64_t)1 << 32)
        return fail(HAKAI_ERR_ARG, "upload_model: %lld nodes exceed one context's 32-bit element-kernel offsets "
                    "(max %lld); split the mesh over ranks", (long long)nNode, (long long)(((int64_t)1 << 32) / 24 - 1));
    HIPCHK(hipSetDevice(c->device));
    (void)hipStreamSynchronize(c->stream);
    hkc::history_destroy(c);  // its buffers are sized for the previous mesh: enable again
    hkc::elem_history_destroy(c);  // so are the element-set history's: enable again
    hkc::stable_dt_destroy(c);  // so is the stable-step scratch: the next call allocates it
    hkc::mass_scale_destroy(c);  // a new model starts unscaled (d_mass is uploaded again below)
    hkc::free_model(c);
    // BC tables are sized for the previous mesh (the fused-BC per-dof table has 3nN entries): a new
    // model starts without BCs until hakai_set_bc runs again
    c->bc = {};
    const long long nN = nNode, nE = nElement;
    const long long nEp = ((nE + 31) / 32) * 32;  // whole 32-element batches; padding behaves as deleted
    // host-side conversions
    std::vector<int> conn((size_t)(8 * nEp), 0), mat((size_t)nEp, 0);
    for (long long e = 0; e < nE; ++e) {
        for (int i = 0; i < 8; ++i) {
            const int64_t n = elementmat[8 * e + i];
            if (n < 1 || n > nN) return fail(HAKAI_ERR_ARG, "elementmat[%d,%lld] = %lld out of 1..%lld", i + 1, e + 1, (long long)n, nN);
            conn[8 * e + i] = (int)(n - 1);
        }
        const int64_t m = element_material[e];
        if (m < 1 || m > nMat) return fail(HAKAI_ERR_ARG, "element_material[%lld] = %lld out of 1..%d", e + 1, (long long)m, nMat);
        mat[e] = (int)(m - 1);
    }
    std::vector<double> mass((size_t)nN);
    for (long long n = 0; n < nN; ++n) {
        const double m0 = diag_M[3 * n], m1 = diag_M[3 * n + 1], m2 = diag_M[3 * n + 2];
        if (!(m0 == m1 && m1 == m2))
            return fail(HAKAI_ERR_ARG, "diag_M: node %lld has different masses per dof", n + 1);
        mass[n] = m0;
    }
    c->h_mats.assign((size_t)nMat, DevMat());
    c->nmat = nMat;
    c->has_ductile = false;
    for (int i = 0; i < nMat; ++i) {
        int r = hkc::build_devmat(mats[i], c->h_mats[i]);
        if (r) return r;
    }
    c->any_plastic = false;
    for (long long e = 0; e < nE; ++e) {
        if (c->h_mats[mat[e]].nd > 0) c->has_ductile = true;
        if (c->h_mats[mat[e]].npp > 0) c->any_plastic = true;
    }
    // node -> (8e+i) incidence CSR in ascending element order (counting sort keeps the order)
    std::vector<int> ptr((size_t)nN + 1, 0), inc((size_t)(8 * nE));
    for (long long j = 0; j < 8 * nE; ++j) ptr[conn[j] + 1]++;
    for (long long n = 0; n < nN; ++n) ptr[n + 1] += ptr[n];
    {
        std::vector<int> fill(ptr.begin(), ptr.end() - 1);
        for (long long j = 0; j < 8 * nE; ++j) inc[fill[conn[j]]++] = (int)j;
    }
    int maxinc = 0;
    for (long long n = 0; n < nN; ++n) maxinc = std::max(maxinc, ptr[n + 1] - ptr[n]);
    c->nN = nN;
    c->nE = nE;
    c->nEp = nEp;
    c->ld = 8 * nEp;
    const size_t ld = (size_t)c->ld;
    HIPCHK(c->d_coord.alloc(3 * (size_t)nN));
    HIPCHK(c->d_u[0].alloc(3 * (size_t)nN));
    HIPCHK(c->d_u[1].alloc(3 * (size_t)nN));
    HIPCHK(c->d_mass.alloc((size_t)nN));
    HIPCHK(c->d_conn.alloc(8 * (size_t)nEp));
    HIPCHK(c->d_flag.alloc((size_t)nEp));
    HIPCHK(c->d_mat.alloc((size_t)nEp));
    HIPCHK(c->d_del_step.alloc((size_t)nEp + 2));
    HIPCHK(c->d_mats.alloc((size_t)nMat));
    HIPCHK(c->d_stress.alloc(6 * ld));
    HIPCHK(c->d_strain.alloc(6 * ld));
    HIPCHK(c->d_eqps.alloc(ld));
    HIPCHK(c->d_yield.alloc(ld));
    HIPCHK(c->d_triax.alloc(ld));
    // forces: 24nEp doubles in either layout, then zeros up to 26nEp (padding base 24nEp with
    // component stride up to nEp)
    c->fe_len = 26 * nEp + 8;
    HIPCHK(c->d_fe.alloc((size_t)c->fe_len));
    HIPCHK(c->d_inc_ptr.alloc((size_t)nN + 1));
    HIPCHK(c->d_inc.alloc(8 * (size_t)nE));
    HIPCHK(c->d_inc_row.alloc(8 * (size_t)nE));
    HIPCHK(c->d_qbuf.alloc(3 * (size_t)nN));
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(c->d_coord, coordmat, 3 * nN * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_mass, mass.data(), nN * sizeof(double), hipMemcpyHostToDevice, s));
    if (nE) {
        HIPCHK(hipMemcpyAsync(c->d_conn, conn.data(), 8 * nEp * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->d_mat, mat.data(), nEp * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->d_inc_row, inc.data(), 8 * nE * sizeof(int), hipMemcpyHostToDevice, s));
    }
    {  // connectivity templates: base node + shared offset pattern, where the mesh has few patterns
        hk::ConnPlan cp;
        if (nE && hk::conn_plan(conn.data(), nEp, cp)) {
            std::vector<unsigned> rp(cp.rec);  // the records, then the table
            rp.insert(rp.end(), cp.pat.begin(), cp.pat.end());
            HIPCHK(c->d_conn_rec.upload(rp, s));
            HIPCHK(hipStreamSynchronize(s));  // (rp goes out of scope)
            c->conn_P = cp.P;
            c->conn_bits = cp.base_bits;
            c->conn_bytes = cp.bytes;
        }
    }
    HIPCHK(hipMemcpyAsync(c->d_mats, c->h_mats.data(), nMat * sizeof(DevMat), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_inc_ptr, ptr.data(), (nN + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    if (maxinc <= 8) HIPCHK(c->d_inc8.alloc(8 * (size_t)nN));  // padded table for the unrolled gather
    HIPCHK(hipStreamSynchronize(s));  // host vectors go out of scope
    c->max_inc = maxinc;
    c->h_ptr = ptr;
    c->h_inc0 = inc;
    {
        int r = fe_upload_incidence(c);
        if (r) return r;
    }
    c->h_coord.assign(coordmat, coordmat + 3 * nN);
    c->h_conn.assign(conn.begin(), conn.begin() + 8 * nE);
    c->h_mat.assign(mat.begin(), mat.begin() + nE);
    c->h_young.resize((size_t)nMat);
    for (int i = 0; i < nMat; ++i) c->h_young[i] = mats[i].young;
    c->h_poisson.resize((size_t)nMat);
    for (int i = 0; i < nMat; ++i) c->h_poisson[i] = mats[i].poisson;
    c->model_ok = true;
    c->state_ok = false;
    return hakai_reset_state(c, 0, nullptr, nullptr, 1.0);
}

int hakai_set_bc(hakai_ctx* c, const hakai_bc_t* bc) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c || !bc) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "set_bc before upload_model");
    HIPCHK(hipSetDevice(c->device));
    (void)hipStreamSynchronize(c->stream);
    c->bc = {};
    const int G = bc->n_groups;
    if (G <= 0) return hkc::history_bc_changed(c);
    // Resolve in-order overwrites: final writer of each dof (v2/HAKAI_j.jl:585-617).
    std::map<long long, std::pair<int, double>> last;
    for (int g = 0; g < G; ++g) {
        if (bc->amp_n[g] == 1)
            return fail(HAKAI_ERR_MODEL, "BC group %d: one-point amplitude, the reference raises BoundsError (:598)", g + 1);
        for (int64_t en = bc->entry_off[g]; en < bc->entry_off[g + 1]; ++en)
            for (int64_t d = bc->dof_off[en]; d < bc->dof_off[en + 1]; ++d) {
                const int64_t dof = bc->dofs[d];
                if (dof < 1 || dof > 3 * c->nN) return fail(HAKAI_ERR_ARG, "BC dof %lld out of range", (long long)dof);
                last[dof - 1] = std::make_pair(g, bc->entry_value[en]);
            }
    }
    std::vector<int> dof, grp;
    std::vector<double> val;
    for (auto& kv : last) {
        dof.push_back((int)kv.first);
        grp.push_back(kv.second.first);
        val.push_back(kv.second.second);
    }
    std::vector<int> amp_n(G), amp_off(G);
    long long n_amp = 0;
    for (int g = 0; g < G; ++g) {
        amp_n[g] = bc->amp_n[g];
        amp_off[g] = (int)bc->amp_off[g];
        n_amp = std::max<long long>(n_amp, bc->amp_off[g] + bc->amp_n[g]);
    }
    c->bc.n = (int)dof.size();
    HIPCHK(c->bc.d_dof.alloc(dof.size()));
    HIPCHK(c->bc.d_grp.alloc(grp.size()));
    HIPCHK(c->bc.d_val.alloc(val.size()));
    HIPCHK(c->bc.d_amp_n.alloc((size_t)G));
    HIPCHK(c->bc.d_amp_off.alloc((size_t)G));
    HIPCHK(c->bc.d_amp_t.alloc((size_t)n_amp));
    HIPCHK(c->bc.d_amp_v.alloc((size_t)n_amp));
    hipStream_t s = c->stream;
    if (!dof.empty()) {
        HIPCHK(hipMemcpyAsync(c->bc.d_dof, dof.data(), dof.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->bc.d_grp, grp.data(), grp.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->bc.d_val, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(c->bc.d_amp_n, amp_n.data(), G * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->bc.d_amp_off, amp_off.data(), G * sizeof(int), hipMemcpyHostToDevice, s));
    if (n_amp) {
        HIPCHK(hipMemcpyAsync(c->bc.d_amp_t, bc->amp_time, n_amp * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->bc.d_amp_v, bc->amp_value, n_amp * sizeof(double), hipMemcpyHostToDevice, s));
    }
    // per-node table: the first resolved entry of each node (entries are sorted by dof, a node's
    // up-to-3 entries are consecutive) or -1, so the nodal kernel applies the BCs itself
    // (hakai_step; 4 B per node)
    if (!dof.empty()) {  // (used by k_nodal up to kFuseBcMaxNodes, and by the two-step schedule)
        std::vector<int> of((size_t)c->nN, -1);
        for (size_t i = dof.size(); i-- > 0;) of[(size_t)dof[i] / 3] = (int)i;
        HIPCHK(c->bc.d_of_node.alloc(of.size()));
        HIPCHK(hipMemcpyAsync(c->bc.d_of_node, of.data(), of.size() * sizeof(int), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return hkc::history_bc_changed(c);
}

int hakai_reset_state(hakai_ctx* c, int64_t n_ic, const int64_t* ic_dofs, const double* ic_values, double d_time) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "reset_state before upload_model");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t fn = 3 * (size_t)c->nN;
    c->sv.restart(false);  // the next nodal update gathers the zeroed fe
    HIPCHK(hipMemsetAsync(c->d_u[0], 0, fn * sizeof(double), s));
    HIPCHK(hipMemsetAsync(c->d_u[1], 0, fn * sizeof(double), s));
    HIPCHK(hipMemsetAsync(c->d_fe, 0, (size_t)c->fe_len * sizeof(double), s));
    HIPCHK(hipMemsetAsync(c->d_del_step, 0, ((size_t)c->nEp + 2) * sizeof(int), s));
    HIPCHK(hk::launch_reset_gp(c->d_stress, c->d_strain, c->d_eqps, c->d_yield, c->d_triax, c->d_flag, c->d_mat,
                               c->d_mats, c->nE, c->nEp, c->ld, s));
    c->h_velo0.assign(fn, 0.0);
    HIPCHK(hipMemsetAsync(c->d_poison, 0, 2 * sizeof(int), s));
    hkc::comm_reset(c);
    if (n_ic > 0) {
        if (!ic_dofs || !ic_values) return fail(HAKAI_ERR_ARG, "reset_state: null IC arrays");
        std::vector<double> dpre(fn, 0.0);
        for (int64_t j = 0; j < n_ic; ++j) {  // v2/HAKAI_j.jl:233-239
            const int64_t d = ic_dofs[j];
            if (d < 1 || d > (int64_t)fn) return fail(HAKAI_ERR_ARG, "IC dof %lld out of range", (long long)d);
            dpre[d - 1] = -ic_values[j] * d_time;
            c->h_velo0[d - 1] = ic_values[j];
        }
        HIPCHK(hipMemcpyAsync(c->d_u[1 - c->sv.cur], dpre.data(), fn * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    c->state_ok = true;
    if (int r = hkc::contact_state_reset(c, c->h_velo0.data())) return r;
    if (int r = hkc::history_restart(c)) return r;
    if (int r = hkc::elem_history_restart(c)) return r;
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int hakai_upload_state(hakai_ctx* c, const hakai_state_t* st) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c || !st) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "upload_state before upload_model");
    HIPCHK(hipSetDevice(c->device));
    // The next nodal update gathers fe unless the upload brings Q or Qe. After a call whose last
    // steps a contact overflow skipped, owner-computed assembly left the last element step's forces
    // only as node sums (fe is an earlier step's): they become the uploaded Q, the same bits, and an
    // upload that also deletes elements (whose fe rows it would zero) must bring Q or Qe itself.
    if (c->sv.q == QSrc::Own && !c->sv.fe_ok && !st->Q && !st->Qe) {
        bool dels = false;
        for (long long e = 0; st->element_flag && e < c->nE && !dels; ++e) dels = st->element_flag[e] == 0;
        if (dels || c->comm)
            return fail(HAKAI_ERR_STATE, "upload_state: the last element step's forces exist only as owner-computed "
                        "node sums (a contact overflow skipped the call's last step); upload Q (from "
                        "hakai_download_state) or Qe with this state");
        if (int r = hkc::own_materialize(c)) return r;
    }
    c->sv.restart(true);
    hipStream_t s = c->stream;
    const size_t fn = 3 * (size_t)c->nN, nGP = 8 * (size_t)c->nE;
    if (st->disp) HIPCHK(hipMemcpyAsync(c->d_u[c->sv.cur], st->disp, fn * sizeof(double), hipMemcpyHostToDevice, s));
    if (st->disp_pre)
        HIPCHK(hipMemcpyAsync(c->d_u[1 - c->sv.cur], st->disp_pre, fn * sizeof(double), hipMemcpyHostToDevice, s));
    if (st->velo) c->h_velo0.assign(st->velo, st->velo + fn);
    if (st->Q) {
        HIPCHK(hipMemcpyAsync(c->d_qbuf, st->Q, fn * sizeof(double), hipMemcpyHostToDevice, s));
        c->sv.q_uploaded();
    }
    if (st->integ_stress || st->integ_strain) {
        DevBuf<double> tmp;
        HIPCHK(tmp.alloc(6 * nGP));
        if (st->integ_stress) {
            HIPCHK(hipMemcpyAsync(tmp, st->integ_stress, 6 * nGP * sizeof(double), hipMemcpyHostToDevice, s));
            HIPCHK(hk::launch_aos_to_soa6(tmp, c->d_stress, (long long)nGP, c->ld, s));
        }
        if (st->integ_strain) {
            HIPCHK(hipMemcpyAsync(tmp, st->integ_strain, 6 * nGP * sizeof(double), hipMemcpyHostToDevice, s));
            HIPCHK(hk::launch_aos_to_soa6(tmp, c->d_strain, (long long)nGP, c->ld, s));
        }
        HIPCHK(hipStreamSynchronize(s));  // (before tmp goes)
    }
    if (st->integ_yield_stress)
        HIPCHK(hipMemcpyAsync(c->d_yield, st->integ_yield_stress, nGP * sizeof(double), hipMemcpyHostToDevice, s));
    if (st->integ_eq_plastic_strain)
        HIPCHK(hipMemcpyAsync(c->d_eqps, st->integ_eq_plastic_strain, nGP * sizeof(double), hipMemcpyHostToDevice, s));
    if (st->integ_triax_stress)
        HIPCHK(hipMemcpyAsync(c->d_triax, st->integ_triax_stress, nGP * sizeof(double), hipMemcpyHostToDevice, s));
    if (st->element_flag) {
        std::vector<int> f((size_t)c->nE);
        for (long long e = 0; e < c->nE; ++e) f[e] = st->element_flag[e] != 0 ? 1 : 0;
        HIPCHK(hipMemcpyAsync(c->d_flag, f.data(), c->nE * sizeof(int), hipMemcpyHostToDevice, s));
        // deleted before the upload: step unknown (-1), never reported by hakai_deleted, but the
        // faces its deletion exposed are live for contact
        std::vector<int> ds((size_t)c->nE);
        for (long long e = 0; e < c->nE; ++e) ds[e] = f[e] ? 0 : -1;
        HIPCHK(hipMemcpyAsync(c->d_del_step, ds.data(), c->nE * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(c->d_del_step + c->nEp, 0, 2 * sizeof(int), s));  // dump + last-deletion slots
        HIPCHK(hipStreamSynchronize(s));
        // fe of elements uploaded as deleted must not contribute
        bool any = false;
        for (long long e = 0; e < c->nE; ++e) any |= !f[e];
        if (any && !st->Qe) {
            std::vector<double> qe(24 * (size_t)c->nE);
            int r = fe_download_qe(c, qe.data());
            if (r) return r;
            for (long long e = 0; e < c->nE; ++e)
                if (!f[e]) std::fill(qe.begin() + 24 * e, qe.begin() + 24 * (e + 1), 0.0);
            if ((r = fe_upload_qe(c, qe.data()))) return r;
        }
    }
    if (st->Qe) {
        int r = fe_upload_qe(c, st->Qe);
        if (r) return r;
    }
    HIPCHK(hipMemsetAsync(c->d_poison, 0, 2 * sizeof(int), s));
    HIPCHK(hipStreamSynchronize(s));
    hkc::comm_reset(c);
    c->state_ok = true;
    if (int r = hkc::history_restart(c)) return r;
    if (int r = hkc::elem_history_restart(c)) return r;
    if (c->contact) {
        if (int r = hkc::contact_state_reset(c, c->h_velo0.empty() ? nullptr : c->h_velo0.data())) return r;
        HIPCHK(hipStreamSynchronize(s));
    }
    return 0;
}

int hakai_download_state(hakai_ctx* c, hakai_state_t* st) {
    if (!c || !st) return fail(HAKAI_ERR_ARG, "null");
    if (!c->state_ok) return fail(HAKAI_ERR_STATE, "download_state without state");
    if (st->Qe && !c->sv.fe_ok)
        return fail(HAKAI_ERR_STATE, "download_state: Qe is not available after a call whose last steps a contact "
                    "overflow skipped (owner-computed assembly keeps node sums only); Q is -- or step once more");
    if (st->integ_triax_stress && !c->sv.triax_ok)
        return fail(HAKAI_ERR_STATE, "download_state: integ_triax_stress is not available after a call whose last "
                    "steps a contact overflow skipped (it is stored on a call's last step); step once more");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t fn = 3 * (size_t)c->nN, nGP = 8 * (size_t)c->nE;
    HIPCHK(hipStreamSynchronize(s));
    if (st->disp) HIPCHK(hipMemcpyAsync(st->disp, c->d_u[c->sv.cur], fn * sizeof(double), hipMemcpyDeviceToHost, s));
    if (st->disp_pre)
        HIPCHK(hipMemcpyAsync(st->disp_pre, c->d_u[1 - c->sv.cur], fn * sizeof(double), hipMemcpyDeviceToHost, s));
    if (st->velo) {
        if (c->sv.steps_done == 0) {
            std::memcpy(st->velo, c->h_velo0.data(), fn * sizeof(double));
        } else {  // velo = d_disp / d_time with d_disp = disp_new - disp (v2/HAKAI_j.jl:625-628)
            std::vector<double> a(fn), b(fn);
            HIPCHK(hipMemcpyAsync(a.data(), c->d_u[c->sv.cur], fn * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(b.data(), c->d_u[1 - c->sv.cur], fn * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (size_t i = 0; i < fn; ++i) {
                const double dd = a[i] - b[i];
                st->velo[i] = dd / c->last_dt;
            }
        }
    }
    if (st->Q) {
        if (c->sv.q == QSrc::Buf) {
            HIPCHK(hipMemcpyAsync(st->Q, c->d_qbuf, fn * sizeof(double), hipMemcpyDeviceToHost, s));
        } else {
            DevBuf<double> tmp;
            HIPCHK(tmp.alloc(fn));
            if (c->sv.q == QSrc::Own) {  // the last element step's owner-computed sums (fe may be stale)
                const hkc::OwnSums o = hkc::own_sums(c);
                HIPCHK(hk::launch_own_q(o.q, o.rp, o.ridx, o.rows, tmp, c->nN, s));
            } else
                HIPCHK(hk::launch_gather_q(c->d_inc_ptr, c->d_inc, c->d_fe, tmp, c->nN, s));
            HIPCHK(hipMemcpyAsync(st->Q, tmp, fn * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));  // (before tmp goes)
        }
    }
    if (st->integ_stress || st->integ_strain) {
        DevBuf<double> tmp;
        HIPCHK(tmp.alloc(6 * nGP));
        if (st->integ_stress) {
            HIPCHK(hk::launch_soa_to_aos6(c->d_stress, tmp, (long long)nGP, c->ld, s));
            HIPCHK(hipMemcpyAsync(st->integ_stress, tmp, 6 * nGP * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (st->integ_strain) {
            HIPCHK(hk::launch_soa_to_aos6(c->d_strain, tmp, (long long)nGP, c->ld, s));
            HIPCHK(hipMemcpyAsync(st->integ_strain, tmp, 6 * nGP * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    if (st->integ_yield_stress)
        HIPCHK(hipMemcpyAsync(st->integ_yield_stress, c->d_yield, nGP * sizeof(double), hipMemcpyDeviceToHost, s));
    if (st->integ_eq_plastic_strain)
        HIPCHK(hipMemcpyAsync(st->integ_eq_plastic_strain, c->d_eqps, nGP * sizeof(double), hipMemcpyDeviceToHost, s));
    if (st->integ_triax_stress)
        HIPCHK(hipMemcpyAsync(st->integ_triax_stress, c->d_triax, nGP * sizeof(double), hipMemcpyDeviceToHost, s));
    if (st->element_flag) {
        std::vector<int> f((size_t)c->nE);
        HIPCHK(hipMemcpyAsync(f.data(), c->d_flag, c->nE * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (long long e = 0; e < c->nE; ++e) st->element_flag[e] = (f[e] == 1) ? 1 : 0;
    }
    if (st->Qe) {
        int r = fe_download_qe(c, st->Qe);
        if (r) return r;
    }
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int hakai_stat(hakai_ctx* c, const char* key, int64_t* value) {
    if (!c || !key || !value) return fail(HAKAI_ERR_ARG, "null");
    if (!std::strcmp(key, "graph_steps")) *value = c->graph_steps;
    else if (!std::strcmp(key, "device_buffers")) *value = hkc::g_dev_live.load();
    else if (!std::strcmp(key, "exchange_retries")) *value = c->exchange_retries;
    else if (!std::strncmp(key, "own_", 4) || !std::strncmp(key, "conn_", 5)) return hkc::own_stat(c, key, value);
    else return fail(HAKAI_ERR_ARG, "unknown stat '%s'", key);
    return 0;
}

int hakai_sync(hakai_ctx* c) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hakai_deleted(hakai_ctx* c, int64_t* n_deleted, int64_t* log, int64_t cap) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "deleted before upload_model");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int> ds((size_t)c->nE);
    if (c->nE) HIPCHK(hipMemcpyAsync(ds.data(), c->d_del_step, c->nE * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // (step, element) in the reference's print order: by step, then element (v2/HAKAI_j.jl:701-736)
    std::vector<std::pair<long long, long long>> v;
    for (long long e = 0; e < c->nE; ++e)
        if (ds[e] > 0) v.push_back(std::make_pair((long long)ds[e], e + 1 + c->elem_offset));
    std::sort(v.begin(), v.end());
    if (n_deleted) *n_deleted = (int64_t)v.size();
    if (log)
        for (long long i = 0; i < (long long)v.size() && i < cap; ++i) {
            log[2 * i] = v[i].first;
            log[2 * i + 1] = v[i].second;
        }
    return 0;
}

int hakai_set_tuning(hakai_ctx* c, const char* key, int64_t value) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c || !key) return fail(HAKAI_ERR_ARG, "set_tuning: null");
    if (!std::strcmp(key, "elem_pipe_blocks")) {
        if (value < 0 || value > 65536) return fail(HAKAI_ERR_ARG, "elem_pipe_blocks out of range");
        c->pipe_blocks = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "elem_gp_nt")) {
        if (value != 0 && value != 1) return fail(HAKAI_ERR_ARG, "elem_gp_nt must be 0 or 1");
        c->gp_nt = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "fuse_bc")) {
        if (value < 0 || value > 2) return fail(HAKAI_ERR_ARG, "fuse_bc must be 0, 1 or 2 (any mesh size)");
        c->fuse_bc = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "elem_pipe_min")) {
        if (value < 0 || value > 1024) return fail(HAKAI_ERR_ARG, "elem_pipe_min out of range");
        c->pipe_min = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "elem_exact")) {
        if (value != 0 && value != 1) return fail(HAKAI_ERR_ARG, "elem_exact must be 0 or 1");
        if (c->elem_exact != (int)value)  // the owner-assembly plan was sized for the other kernel
            if (int r = hkc::own_tuning(c, key, value)) return r;
        c->elem_exact = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "group_serial")) {  // timing: hakai_step_group drains each rank's phase
        if (value < 0 || value > 2) return fail(HAKAI_ERR_ARG, "group_serial must be 0, 1 or 2");
        c->group_serial = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "nodal_padded")) {
        if (!value) {
            c->d_inc8.free();
            return 0;
        }
        return c->d_inc8 ? 0 : fail(HAKAI_ERR_STATE, "padded incidence table unavailable (>8 incidences)");
    }
    if (!std::strncmp(key, "own_", 4)) return hkc::own_tuning(c, key, value);
    if (!std::strcmp(key, "conn_templates")) {  // (every tuning call drops the captured graphs, above)
        if (value != 0 && value != 1) return fail(HAKAI_ERR_ARG, "conn_templates must be 0 or 1");
        c->conn_templates = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "graph")) {
        if (value < 0 || value > 1024 || (value & 1)) return fail(HAKAI_ERR_ARG, "graph must be 0 or an even step count <= 1024");
        c->graph = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "history_one_block")) {  // the history reduction in one launch / two
        if (value < -1 || value > 1) return fail(HAKAI_ERR_ARG, "history_one_block must be -1 (by size), 0 or 1");
        c->hist_one_block = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "elem_history_one_block")) {  // the element-set history's reduction in one launch / two
        if (value < -1 || value > 1) return fail(HAKAI_ERR_ARG, "elem_history_one_block must be -1 (by size), 0 or 1");
        c->ehist_one_block = (int)value;
        return 0;
    }
    if (!std::strncmp(key, "contact_", 8)) {
        HIPCHK(hipSetDevice(c->device));
        return hkc::contact_tuning(c, key, value);
    }
    return fail(HAKAI_ERR_ARG, "unknown tuning key '%s'", key);
}

int hakai_set_element_offset(hakai_ctx* c, int64_t element_offset) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c || element_offset < 0) return fail(HAKAI_ERR_ARG, "set_element_offset: bad args");
    c->elem_offset = element_offset;
    return 0;
}

int hakai_negative_jacobians(hakai_ctx* c, int64_t* n) {
    if (!c || !n) return fail(HAKAI_ERR_ARG, "null");
    if (!c->state_ok) return fail(HAKAI_ERR_STATE, "negative_jacobians without state");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(c->d_negjac, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(hk::launch_negjac(hkc::elem_args(c, c->sv.cur), c->d_negjac, c->stream));
    unsigned long long v = 0;
    HIPCHK(hipMemcpyAsync(&v, c->d_negjac, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n = (int64_t)v;
    return 0;
}

int hakai_node_stress_strain(hakai_ctx* c, double* node_stress, double* node_strain, double* node_eqps,
                             double* node_mises, double* node_triax) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->state_ok) return fail(HAKAI_ERR_STATE, "node_stress_strain without state");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t nN = (size_t)c->nN;
    DevBuf<double> ns, nn, ne, nm, nt;
    HIPCHK(ns.alloc(6 * nN));
    HIPCHK(nn.alloc(6 * nN));
    HIPCHK(ne.alloc(nN));
    HIPCHK(nm.alloc(nN));
    HIPCHK(nt.alloc(nN));
    HIPCHK(hk::launch_node_average(c->d_inc_ptr, c->d_inc_row, c->d_stress, c->d_strain, c->d_eqps, c->d_triax, c->ld,
                                   c->nN, ns, nn, ne, nm, nt, s));
    if (node_stress) HIPCHK(hipMemcpyAsync(node_stress, ns, 6 * nN * sizeof(double), hipMemcpyDeviceToHost, s));
    if (node_strain) HIPCHK(hipMemcpyAsync(node_strain, nn, 6 * nN * sizeof(double), hipMemcpyDeviceToHost, s));
    if (node_eqps) HIPCHK(hipMemcpyAsync(node_eqps, ne, nN * sizeof(double), hipMemcpyDeviceToHost, s));
    if (node_mises) HIPCHK(hipMemcpyAsync(node_mises, nm, nN * sizeof(double), hipMemcpyDeviceToHost, s));
    if (node_triax) HIPCHK(hipMemcpyAsync(node_triax, nt, nN * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int hakai_profile_enable(hakai_ctx* c, int on) { return hakai_profile_mask(c, on ? (1u << HAKAI_K_COUNT) - 1 : 0u); }

int hakai_profile_mask(hakai_ctx* c, uint32_t mask) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!mask) prof_harvest(c);
    c->prof = mask != 0;
    c->prof_mask = mask;
    for (int k = 0; k < HAKAI_K_COUNT; ++k) {
        c->k_ms[k] = 0;
        c->k_n[k] = 0;
    }
    return 0;
}

int hakai_profile_read(hakai_ctx* c, int kernel, double* total_ms, int64_t* launches) {
    if (!c || kernel < 0 || kernel >= HAKAI_K_COUNT) return fail(HAKAI_ERR_ARG, "bad profile query");
    (void)hipSetDevice(c->device);
    prof_harvest(c);
    if (total_ms) *total_ms = c->k_ms[kernel];
    if (launches) *launches = c->k_n[kernel];
    return 0;
}

// ---- stateless literal drop-ins -----------------------------------------------------------------
int hakai_stress_hexa(int device, int64_t nNode, int64_t nElement, double* Qe, double* integ_stress,
                      double* integ_strain, double* integ_yield_stress, double* integ_eq_plastic_strain,
                      const double* position, const double* d_disp, const int64_t* elementmat,
                      const int64_t* element_flag, int32_t integ_num, int32_t nMat, const hakai_material_t* mats,
                      const int64_t* element_material, double* elementVolume) {
    if (integ_num != 8) return fail(HAKAI_ERR_ARG, "integ_num must be 8 (v2/HAKAI_j.jl:177)");
    if (!Qe || !integ_stress || !integ_strain || !integ_yield_stress || !integ_eq_plastic_strain || !position ||
        !d_disp || !element_flag)
        return fail(HAKAI_ERR_ARG, "stress_hexa: null array");
    hakai_ctx* c = nullptr;
    int r = hakai_create(&c, device);
    if (r) return r;
    struct Guard {
        hakai_ctx* c;
        ~Guard() { hakai_destroy(c); }
    } guard{c};
    // position = coord + 0 and d_disp = 0 - (-d_disp): the element kernel reproduces both exactly
    std::vector<double> ones(3 * (size_t)nNode, 1.0);
    r = hakai_upload_model(c, nNode, position, nElement, elementmat, element_material, nMat, mats, ones.data());
    if (r) return r;
    std::vector<double> zero(3 * (size_t)nNode, 0.0), mdu(3 * (size_t)nNode);
    for (size_t i = 0; i < mdu.size(); ++i) mdu[i] = -d_disp[i];
    hakai_state_t st;
    std::memset(&st, 0, sizeof st);
    st.disp = zero.data();
    st.disp_pre = mdu.data();
    st.integ_stress = integ_stress;
    st.integ_strain = integ_strain;
    st.integ_yield_stress = integ_yield_stress;
    st.integ_eq_plastic_strain = integ_eq_plastic_strain;
    st.element_flag = const_cast<int64_t*>(element_flag);
    r = hakai_upload_state(c, &st);
    if (r) return r;
    hipStream_t s = c->stream;
    DevBuf<double> d_vol;
    HIPCHK(d_vol.alloc((size_t)c->nEp));
    HIPCHK(hipMemsetAsync(c->d_fe, 0, 24 * (size_t)nElement * sizeof(double), s));
    hk::ElemArgs ea = hkc::elem_args(c, c->sv.cur);
    ea.vol = d_vol;
    ea.pipe_blocks = 0;
    HIPCHK(hk::launch_element(ea, false, false, s));
    std::vector<double> fe(24 * (size_t)nElement), vol((size_t)nElement);
    HIPCHK(hipMemcpyAsync(fe.data(), c->d_fe, fe.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(vol.data(), d_vol, vol.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    hakai_state_t out;
    std::memset(&out, 0, sizeof out);
    out.integ_stress = integ_stress;
    out.integ_strain = integ_strain;
    out.integ_yield_stress = integ_yield_stress;
    out.integ_eq_plastic_strain = integ_eq_plastic_strain;
    r = hakai_download_state(c, &out);
    if (r) return r;
    for (int64_t e = 0; e < nElement; ++e) {
        if (element_flag[e] == 0) continue;
        for (int j = 0; j < 24; ++j) Qe[24 * e + j] += fe[24 * e + j];
        if (elementVolume) elementVolume[e] = vol[e];
    }
    return 0;
}

int hakai_triax_stress(int device, int64_t nGP, const double* integ_stress, double* integ_triax_stress) {
    if (nGP < 0 || (nGP > 0 && (!integ_stress || !integ_triax_stress))) return fail(HAKAI_ERR_ARG, "triax: bad args");
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= device || device < 0)
        return fail(HAKAI_ERR_DEVICE, "no HIP device %d: no CPU fallback", device);
    HIPCHK(hipSetDevice(device));
    if (nGP == 0) return 0;
    DevBuf<double> st, tx;
    HIPCHK(st.alloc(6 * (size_t)nGP));
    HIPCHK(tx.alloc((size_t)nGP));
    HIPCHK(hipMemcpy(st, integ_stress, 6 * nGP * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hk::launch_triax_aos(st, tx, nGP, 0));
    HIPCHK(hipMemcpy(integ_triax_stress, tx, nGP * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// accessors used by other translation units of the library
namespace hkc {
long long ctx_nN(hakai_ctx* c) { return c->nN; }
}
