// hakai_elem_exact.hpp -- the reference-order element step (ElemArgs::exact 1), with its ordered
// LDS sums over the Gauss points and the diagnostic phase clocks. Device code, included by
// hakai_element.hip only.
#pragma once
#include "hakai_elem_io.hpp"
#include "hakai_exact_math.hpp"

namespace hk {

// ---------------------------------------------------------------------------------------------
// Reference-order element update (tuning key "elem_exact"): cal_stress_hexa's own arithmetic
// (the oracle's restatement: oracle/hakai_oracle.c cal_BVbar_hexa, cal_Bfinal, stress_one_element),
// so the Gauss-point state, the element forces and -- with the bit-exact nodal update and contact --
// whole trajectories are the reference's bits. Same mapping as elem_step (lane k = Gauss point k),
// no contraction, fma exactly where the reference's StaticArrays products use muladd:
//   * Jacobian of GP k summed in node order 1..8 (:1424-1434) from the Pusai table (cal_Pusai_hexa,
//     built on the host with the reference's expression), cofactor det/inverse (:1436-1455), and
//     P2 = dN_i/dx (:1457-1470), computed ONCE per GP: cal_BVbar_hexa (:1716-1754) forms the same
//     P2 with 1/|det| and weights it with |det|, which is (P2/3)*det with the signed det, bit for bit;
//   * BVbar[:, 3i+c] = (sum over GPs in order of (P2/3)*|det|) / V, V = sum |det| (:1729-1780): each
//     lane writes its 8 node terms to an LDS exchange area, lane i sums node i's column over the 8
//     lanes in GP order;
//   * Bfinal (:1472-1490) is never stored: its entries are Pix, Piy, Piz, t = BVbar - P2/3 (kept in
//     registers, one division by 3 per entry) and structural zeros, fed to the 6x24 * 24 chain (:1204)
//     column by column in the reference's order; the same for D*de (:1205) and Bfinal'*sigma
//     (:1330-1340). A structural zero term is fma(0, x, acc) == acc unless acc is a zero, so dropping
//     it can change only the SIGN of a zero intermediate; every stored quantity is a sum started
//     from +0 or a previous value that is never -0, so the stored bits are the same
//     (tests/test_exact_chains.py checks the chains on ±0-rich inputs);
//   * radial return with the reference's divisions (:1251-1282): x/3 and a/q are correctly rounded
//     by div3 / div_cr below (same bits as IEEE division, fewer instructions);
//   * Qe[:, e] += detJ * Bfinal' * sigma summed over the GPs in order through the exchange area;
//     deletion averages (:701-712) summed in GP order; triaxiality in invariant form (the
//     reference's eigvals agree to rounding; it only enters the deletion test and the output).
// ---------------------------------------------------------------------------------------------

// x/3 and a/b correctly rounded without IEEE division sequences: div3 and div_cr, with the
// hardening-segment search and the ductile table, live in hakai_exact_math.hpp (host and device;
// the CPU tests compile that header).

// Ordered sum over the 8 Gauss points (lanes) of an element, for every node at once: lane k
// contributes v[i] for node i; lane i returns ((v_0[i] + v_1[i]) + ...) + v_7[i] (GP order, from
// +0 like the reference's zero-initialised accumulators). w: the element's exchange area.
__device__ __forceinline__ double gp_sum8(double* w, int k, const double (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w[8 * i + k] = v[i];
    wave_lds_fence();
    double r[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) r[kk] = w[8 * k + kk];
    wave_lds_fence();
    double acc = 0.0 + r[0];
#pragma unroll
    for (int kk = 1; kk < 8; ++kk) acc += r[kk];
    return acc;
}

// Ordered sum over the 8 lanes of a scalar (one LDS round trip); every lane gets it.
__device__ __forceinline__ double gp_all8(double* w, int k, double x) {
    w[k] = x;
    wave_lds_fence();
    double r[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) r[kk] = w[kk];
    wave_lds_fence();
    double a = 0.0 + r[0];
#pragma unroll
    for (int kk = 1; kk < 8; ++kk) a += r[kk];
    return a;
}

// Diagnostic build only (-DHK_DIAG_PHASE, tools/diag_wave.py): per-wave clock totals of the phases of
// the reference-order element step (sched_barrier pins each stamp between the phases it separates).
#ifdef HK_DIAG_PHASE
struct PhaseClock {
    long long t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long last = 0;
};
#define HK_PH(pc, i)                                   \
    do {                                               \
        __builtin_amdgcn_sched_barrier(0);             \
        const long long now_ = clock64();              \
        (pc).t[i] += now_ - (pc).last;                 \
        (pc).last = now_;                              \
        __builtin_amdgcn_sched_barrier(0);             \
    } while (0)
#define HK_PH_ARG , PhaseClock& pc
#define HK_PH_PASS , pc
#else
#define HK_PH(pc, i) \
    do {             \
    } while (0)
#define HK_PH_ARG
#define HK_PH_PASS
#endif

template <bool DO_DELETE, bool STORE_TRIAX, bool ANY_PLASTIC, bool WITH_VOL, int NT = 0, bool OWN = false>
__device__ __forceinline__ void elem_step_exact(const ElemArgs& a, const DevMat* __restrict__ mats, long long e,
                                                int k, double* nd8, double* xb, const double* pus,
                                                const ElemIn& in, double* sfe HK_PH_ARG) {
#pragma clang fp contract(off)
    const DevMat* M = mats + in.mt;
    const bool active = in.fl == 1;
    const int npp = M->npp;
    const int nd = DO_DELETE ? M->nd : 0;
    double eqp = in.eqp, ys = in.ys;

    // position = coord + u, d_disp = u - u_pre (load_node's expressions) from the raw loads
    nd8[6 * k + 0] = in.cx[0] + in.uu[0];
    nd8[6 * k + 1] = in.cx[1] + in.uu[1];
    nd8[6 * k + 2] = in.cx[2] + in.uu[2];
    nd8[6 * k + 3] = in.uu[0] - in.up[0];
    nd8[6 * k + 4] = in.uu[1] - in.up[1];
    nd8[6 * k + 5] = in.uu[2] - in.up[2];
    wave_lds_fence();
    HK_PH(pc, 1);

    // ---- Jacobian at GP k in node order, det and inverse (cal_Bfinal :1424-1455; cal_BVbar_hexa
    // computes the same J and det at :1716-1740). The first term starts the sum (0 + x == x).
    const double* P0 = pus + kPusStride * k;  // Pusai_mat[k][r][i] = pus[26k + 8r + i] (stage_pusai pads)
    const double* P1 = P0 + 8;
    const double* P2 = P0 + 16;
    double J11, J12, J13, J21, J22, J23, J31, J32, J33;
    {
        const double X0 = nd8[0], X1 = nd8[1], X2 = nd8[2];
        J11 = P0[0] * X0; J12 = P0[0] * X1; J13 = P0[0] * X2;
        J21 = P1[0] * X0; J22 = P1[0] * X1; J23 = P1[0] * X2;
        J31 = P2[0] * X0; J32 = P2[0] * X1; J33 = P2[0] * X2;
    }
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        const double X0 = nd8[6 * i + 0], X1 = nd8[6 * i + 1], X2 = nd8[6 * i + 2];
        J11 += P0[i] * X0;
        J12 += P0[i] * X1;
        J13 += P0[i] * X2;
        J21 += P1[i] * X0;
        J22 += P1[i] * X1;
        J23 += P1[i] * X2;
        J31 += P2[i] * X0;
        J32 += P2[i] * X1;
        J33 += P2[i] * X2;
    }
    const double v = J11 * J22 * J33 + J12 * J23 * J31 + J13 * J21 * J32 - J11 * J23 * J32 - J12 * J21 * J33 -
                     J13 * J22 * J31;
    const double div_v = 1.0 / v;
    double pd[8][3];  // P2 = dN_i/dx at GP k (:1457-1470)
    {
        const double iJ11 = (J22 * J33 - J23 * J32) * div_v;
        const double iJ21 = (J23 * J31 - J21 * J33) * div_v;
        const double iJ31 = (J21 * J32 - J22 * J31) * div_v;
        const double iJ12 = (J13 * J32 - J12 * J33) * div_v;
        const double iJ22 = (J11 * J33 - J13 * J31) * div_v;
        const double iJ32 = (J12 * J31 - J11 * J32) * div_v;
        const double iJ13 = (J12 * J23 - J13 * J22) * div_v;
        const double iJ23 = (J13 * J21 - J11 * J23) * div_v;
        const double iJ33 = (J11 * J22 - J12 * J21) * div_v;
        // pd[i][r] = iJr1 * P0[i] + iJr2 * P1[i] + iJr3 * P2[i]. The Pusai table is odd in the node's
        // r-th sign, ((1/8 * delta_r) * f) * g with delta_r = +-1 (hkc::pusai_table), so
        // Pusai[k][r][i] == -Pusai[k][r][partner_r(i)] bit for bit with partner_r flipping that sign
        // (i^1, i^3, i^4 in C3D8 order); RN(-x) = -RN(x), so each product is formed once per
        // partner pair and the sums take it with a sign modifier: the same bits, 36 fewer multiplies.
        auto row = [&](int r, double a, double b, double c) {
            double q0[8], q1[8], q2[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!(((i + 1) >> 1) & 1)) q0[i] = a * P0[i];
                if (!((i >> 1) & 1)) q1[i] = b * P1[i];
                if (!((i >> 2) & 1)) q2[i] = c * P2[i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double s0 = (((i + 1) >> 1) & 1) ? -q0[i ^ 1] : q0[i];
                const double s1 = ((i >> 1) & 1) ? -q1[i ^ 3] : q1[i];
                const double s2 = ((i >> 2) & 1) ? -q2[i ^ 4] : q2[i];
                pd[i][r] = s0 + s1 + s2;
            }
        };
        row(0, iJ11, iJ12, iJ13);
        row(1, iJ21, iJ22, iJ23);
        row(2, iJ31, iJ32, iJ33);
    }

    HK_PH(pc, 2);
    // P2/3 (cal_BVbar_hexa's P2 / 3 at :1745-1750 and Bfinal's -P2/3 at :1482-1490: the same
    // correctly rounded quotient), formed once; it becomes t(i,c) below, in place
    double tk[8][3];
    // ---- V and BVbar (:1729-1780)
    double V;  // sum of |det| in GP order, in the first component's round trip
    {
        // software-pipelined: a component's exchange reads are in flight while the next
        // component's P2/3 and terms are formed (C3 exact element 1.083 -> 1.077 ms, one box)
        auto comp = [&](int c, double (&w)[8]) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                tk[i][c] = div3(pd[i][c]);
                w[i] = tk[i][c] * v;
            }
        };
        auto sum = [&](const double (&r)[8]) {
            double acc = 0.0 + r[0];
#pragma unroll
            for (int kk = 1; kk < 8; ++kk) acc += r[kk];
            return acc;
        };
        double w[8], r[8], bs[3];
        comp(0, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) xb[8 * i + k] = w[i];
        xb[64 + k] = fabs(v);
        wave_lds_fence();
        double q[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) r[kk] = xb[8 * k + kk];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) q[kk] = xb[64 + kk];
        wave_lds_fence();
        comp(1, w);
        bs[0] = sum(r);
        V = sum(q);
#pragma unroll
        for (int i = 0; i < 8; ++i) xb[8 * i + k] = w[i];
        wave_lds_fence();
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) r[kk] = xb[8 * k + kk];
        wave_lds_fence();
        comp(2, w);
        bs[1] = sum(r);
#pragma unroll
        for (int i = 0; i < 8; ++i) xb[8 * i + k] = w[i];
        wave_lds_fence();
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) r[kk] = xb[8 * k + kk];
        wave_lds_fence();
        bs[2] = sum(r);
        const double rV = 1.0 / V;
#pragma unroll
        for (int c = 0; c < 3; ++c) nd8[6 * k + c] = div_cr(bs[c], V, rV);
    }
    wave_lds_fence();
    // Bfinal rows 1-3 carry t(i,c) = -P2/3 + BVbar (:1482-1490), formed once per node and component
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) tk[i][c] = nd8[6 * i + c] - tk[i][c];
    auto tq = [&](int i, int c) { return tk[i][c]; };
    HK_PH(pc, 3);

    // ---- de = Bfinal * d_u (:1204): per row, the fma chain over columns j = 3i+c in order.
    // Bfinal column (i,c) by rows: c=0: (Pix+t0, t0, t0, Piy, 0, Piz); c=1: (t1, Piy+t1, t1, Pix,
    // Piz, 0); c=2: (t2, t2, Piz+t2, 0, Piy, Pix).
    double de[6];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double* D = nd8 + 6 * i + 3;
        const double u0 = D[0], u1 = D[1], u2 = D[2];
        const double t0 = tq(i, 0), t1 = tq(i, 1), t2 = tq(i, 2);
        const double px = pd[i][0], py = pd[i][1], pz = pd[i][2];
        if (i == 0) {
            de[0] = (px + t0) * u0;
            de[1] = t0 * u0;
            de[2] = t0 * u0;
            de[3] = py * u0;
            de[4] = pz * u1;  // column 0 of row 5 is a structural zero
            de[5] = pz * u0;
        } else {
            de[0] = __builtin_fma(px + t0, u0, de[0]);
            de[1] = __builtin_fma(t0, u0, de[1]);
            de[2] = __builtin_fma(t0, u0, de[2]);
            de[3] = __builtin_fma(py, u0, de[3]);
            de[5] = __builtin_fma(pz, u0, de[5]);
            de[4] = __builtin_fma(pz, u1, de[4]);
        }
        de[0] = __builtin_fma(t1, u1, de[0]);
        de[1] = __builtin_fma(py + t1, u1, de[1]);
        de[2] = __builtin_fma(t1, u1, de[2]);
        de[3] = __builtin_fma(px, u1, de[3]);
        de[0] = __builtin_fma(t2, u2, de[0]);
        de[1] = __builtin_fma(t2, u2, de[1]);
        de[2] = __builtin_fma(pz + t2, u2, de[2]);
        de[4] = __builtin_fma(py, u2, de[4]);
        de[5] = __builtin_fma(px, u2, de[5]);
        asm volatile("" ::: "memory");  // one node's LDS operands in flight at a time (VGPRs)
    }

    HK_PH(pc, 4);
    // ---- d_o = Dmat * de (:1205): the 6x6 chain without its structural zeros
    const double Dn = M->Dn, Do = M->Do, Ds = M->Ds;
    double fin[6];
    fin[0] = in.sig[0] + __builtin_fma(Do, de[2], __builtin_fma(Do, de[1], Dn * de[0]));
    fin[1] = in.sig[1] + __builtin_fma(Do, de[2], __builtin_fma(Dn, de[1], Do * de[0]));
    fin[2] = in.sig[2] + __builtin_fma(Dn, de[2], __builtin_fma(Do, de[1], Do * de[0]));
    fin[3] = in.sig[3] + Ds * de[3];
    fin[4] = in.sig[4] + Ds * de[4];
    fin[5] = in.sig[5] + Ds * de[5];
    // ---- J2 radial return (:1227-1289)
    if (ANY_PLASTIC && npp > 0) {
        const double mean = div3(fin[0] + fin[1] + fin[2]);
        const double dev[6] = {fin[0] - mean, fin[1] - mean, fin[2] - mean, fin[3], fin[4], fin[5]};
        const double q = sqrt(1.5 * (dev[0] * dev[0] + dev[1] * dev[1] + dev[2] * dev[2] + 2.0 * (dev[3] * dev[3]) +
                                     2.0 * (dev[4] * dev[4]) + 2.0 * (dev[5] * dev[5])));
        if (q > ys) {
            const int p = plastic_segment(M->pl_eps, npp, eqp);  // (:1255-1264), 0-based
            const double H = M->Hd[p];
            const double dep = (q - ys) / (3.0 * M->G + H);
            const double s = ys + H * dep;
            const double rq = 1.0 / q;
#pragma unroll
            for (int r = 0; r < 3; ++r) fin[r] = div_cr(dev[r] * s, q, rq) + mean;
#pragma unroll
            for (int r = 3; r < 6; ++r) fin[r] = div_cr(dev[r] * s, q, rq) + 0.0;
            eqp = eqp + dep;
            ys = ys + H * dep;
        }
    }
    // ---- triaxiality of the final stress (invariant form of :995-1018; the reference's eigenvalue
    // differences give the same value to rounding -- it enters only the deletion test and the output).
    // Formed where it is stored (a call's last step) or the deletion test needs it (below); an
    // inactive element's value is never used, so forming it after the inactive select changes nothing.
    auto triax = [&]() {
        const double mean = div3(fin[0] + fin[1] + fin[2]);
        const double a01 = fin[0] - fin[1], a12 = fin[1] - fin[2], a20 = fin[2] - fin[0];
        const double oeq = sqrt(0.5 * (a01 * a01 + a12 * a12 + a20 * a20) +
                                3.0 * (fin[3] * fin[3] + fin[4] * fin[4] + fin[5] * fin[5]));
        return (oeq < 1e-10) ? 0.0 : mean / oeq;
    };
    double eps[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) eps[c] = active ? in.eps[c] + de[c] : in.eps[c];
    // inactive elements keep their state (:1116-1118); selected here so the previous state does not
    // stay live through the force pass (their forces are masked at the write-back)
#pragma unroll
    for (int c = 0; c < 6; ++c) fin[c] = active ? fin[c] : in.sig[c];
    if (!active) {
        eqp = in.eqp;
        ys = in.ys;
    }

    HK_PH(pc, 5);
    double tri = STORE_TRIAX ? triax() : 0.0;
    bool kill = false;
    // element averages in GP order (:701-712); a wave whose Gauss points all lie below du_skip has
    // none that can reach the ductile table (wave-uniform skip, the same decisions)
    if (DO_DELETE && nd > 0 && __builtin_amdgcn_ballot_w64(eqp >= M->du_skip) != 0) {
        const double v_e = gp_all8(xb, k, eqp) * 0.125;  // /8, exact
        // below du_floor no fracture strain of the table is reached whatever the triaxiality: the
        // average triaxiality (a second round trip) only where it can matter; the 8 lanes of an
        // element share v_e, so the branch is uniform over them
        if (v_e >= M->du_floor) {
            if (!STORE_TRIAX) tri = triax();
            const double t_e = gp_all8(xb, k, tri) * 0.125;
            if (!(t_e < 0.0)) kill = active && v_e >= ductile_fr(M->du_eps, M->du_tri, nd, t_e);
        }
    }

    // the Gauss-point state, flag and deletion log are final here: stored before the force pass, so
    // their registers are free for it and the stores stream out under its arithmetic
    if (WITH_VOL) a.vol[e] = V;
    {
        const double nofk[3] = {0.0, 0.0, 0.0};
        elem_writeback<DO_DELETE, STORE_TRIAX, ANY_PLASTIC, NT, true, OWN, true, kWbState>(a, e, k, in, active, kill,
                                                                                          nofk, fin, eps, eqp, ys, tri);
    }
    // ---- Qe[:, e] += detJ * Bfinal' * sigma (:1330-1340), GP contributions summed in GP order
    double fk[3];
    {
        double w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // column (i, 0): (Pix+t0, t0, t0, Piy, 0, Piz)
            const double t0 = tq(i, 0);
            double acc = (pd[i][0] + t0) * fin[0];
            acc = __builtin_fma(t0, fin[1], acc);
            acc = __builtin_fma(t0, fin[2], acc);
            acc = __builtin_fma(pd[i][1], fin[3], acc);
            acc = __builtin_fma(pd[i][2], fin[5], acc);
            w[i] = v * acc;  // W*W*W*detJ*acc with W = 1
        }
        fk[0] = gp_sum8(xb, k, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // column (i, 1): (t1, Piy+t1, t1, Pix, Piz, 0)
            const double t1 = tq(i, 1);
            double acc = t1 * fin[0];
            acc = __builtin_fma(pd[i][1] + t1, fin[1], acc);
            acc = __builtin_fma(t1, fin[2], acc);
            acc = __builtin_fma(pd[i][0], fin[3], acc);
            acc = __builtin_fma(pd[i][2], fin[4], acc);
            w[i] = v * acc;
        }
        fk[1] = gp_sum8(xb, k, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // column (i, 2): (t2, t2, Piz+t2, 0, Piy, Pix)
            const double t2 = tq(i, 2);
            double acc = t2 * fin[0];
            acc = __builtin_fma(t2, fin[1], acc);
            acc = __builtin_fma(pd[i][2] + t2, fin[2], acc);
            acc = __builtin_fma(pd[i][1], fin[4], acc);
            acc = __builtin_fma(pd[i][0], fin[5], acc);
            w[i] = v * acc;
        }
        fk[2] = gp_sum8(xb, k, w);
    }
    HK_PH(pc, 6);
    elem_writeback<DO_DELETE, STORE_TRIAX, ANY_PLASTIC, NT, true, OWN, true, kWbForce>(a, e, k, in, active, kill, fk,
                                                                                      fin, eps, eqp, ys, tri, sfe);
    HK_PH(pc, 7);
}

}  // namespace hk
