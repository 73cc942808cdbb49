// hakai_elem_fused.hpp -- the fused element step (ElemArgs::exact 0): hex8 B-bar, J2 radial return,
// internal force, triaxiality and ductile deletion in one pass, free to contract within an
// expression (tolerance-checked). Device code, included by hakai_element.hip only.
#pragma once
#include "hakai_elem_io.hpp"
#include "hakai_exact_math.hpp"

namespace hk {

// ---------------------------------------------------------------------------------------------
// Element update: one 8-lane group per hex8 element, lane k = Gauss point k (gc order of
// v2/HAKAI_j.jl:1913-1920: k bits = (xi, eta, zeta) signs).
//
// Math (identical to the reference's Bfinal algebra, reorganised so no 6x24 matrix is formed):
//   P_k   = J_k^{-1} Pusai_k                    (dN_i/dx at GP k, signed det_k)
//   bbar_i = sum_k det_k P_k[:,i] / (3V),  V = sum_k |det_k|      (= BVbar rows 1-3, :1766-1780)
//   de    = sym(grad du) + (sum_i bbar_i.du_i - div_k(du)/3) (1,1,1,0,0,0)     (= Bfinal*d_u)
//   f_i  += det_k (sigma_k - tr_k/3 I) P_k[:,i] ;  f_i += (sum_k det_k tr sigma_k) bbar_i
//                                                                            (= sum_k det_k Bfinal' sigma)
// ---------------------------------------------------------------------------------------------

// One element step for the 8 lanes of a group (every group runs it; the element flag selects what
// is stored):  flag 1 -> full update;  flag 2 (deleted in the previous step) -> Qe and triaxiality
// become 0 and the flag 0 (the reference skips deleted elements, :1116, and their stress is zero);
// flag 0 -> state written back unchanged, Qe 0.
template <bool DO_DELETE, bool STORE_TRIAX, bool ANY_PLASTIC, bool WITH_VOL, int NT = 0, bool OWN = false>
__device__ __forceinline__ void elem_step(const ElemArgs& a, const DevMat* __restrict__ mats, long long e, int k,
                                          double* nd8, const ElemIn& in, double* sfe = nullptr) {
    const DevMat* M = mats + in.mt;
    const bool active = in.fl == 1;
    const int npp = M->npp;
    const int nd = DO_DELETE ? M->nd : 0;
    double eqp = in.eqp, ys = in.ys;

    // ---- share the 8 nodes of the element through LDS (this 8-lane group only, same wave:
    // LDS operations of one wave complete in order, so a wavefront-scope fence suffices).
    nd8[6 * k + 0] = in.x[0];
    nd8[6 * k + 1] = in.x[1];
    nd8[6 * k + 2] = in.x[2];
    nd8[6 * k + 3] = in.du[0];
    nd8[6 * k + 4] = in.du[1];
    nd8[6 * k + 5] = in.du[2];
    wave_lds_fence();

    // ---- Relative node slots. Label a node by its sign bits s = (x>0)<<2 | (y>0)<<1 | (z>0); GP k
    // carries its (xi, eta, zeta) signs in the same bits (v2/HAKAI_j.jl:1913-1920). Lane k works on
    // slot j = s ^ k: the magnitudes of dN_s/dxi at GP k (cal_Pusai_hexa, :1924-1934) then depend on
    // j only -- (1+g) where node and GP signs agree, (1-g) where they differ -- and the node's own
    // sign is tau_r * sgn(j_r) with the lane constant tau_r = (k_r ? -1 : 1). So J = diag(tau) Jt,
    // det J = tau_x tau_y tau_z det Jt and J^-1 dN_s = Jt^-1 D(j): the tau never appear, and the
    // two reduce-scatters below need no per-lane selects (reduce_scatter8_rel). The node sums run in
    // slot order, a lane-dependent permutation of the reference's node order (rounding only).
    const double g = 1.0 / __builtin_sqrt(3.0);
    const double hp = 1.0 + g, hm = 1.0 - g;
    int nodej[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) nodej[j] = 6 * ref_of_sign(j ^ k);
#define HK_MG(j, b) ((((j) >> (b)) & 1) ? hm : hp)
#define HK_SG(j, b) ((((j) >> (b)) & 1) ? 1.0 : -1.0)
#define HK_D0(j) (HK_SG(j, 2) * (1.0 / 8.0 * HK_MG(j, 1) * HK_MG(j, 0)))
#define HK_D1(j) (HK_SG(j, 1) * (1.0 / 8.0 * HK_MG(j, 2) * HK_MG(j, 0)))
#define HK_D2(j) (HK_SG(j, 0) * (1.0 / 8.0 * HK_MG(j, 2) * HK_MG(j, 1)))
    // ---- Jacobian (:1424-1434), determinant and cofactor inverse (:1436-1455), on Jt
    double J[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double* X = nd8 + nodej[j];
        const double X0 = X[0], X1 = X[1], X2 = X[2];
        const double p0 = HK_D0(j), p1 = HK_D1(j), p2 = HK_D2(j);
        J[0][0] += p0 * X0; J[0][1] += p0 * X1; J[0][2] += p0 * X2;
        J[1][0] += p1 * X0; J[1][1] += p1 * X1; J[1][2] += p1 * X2;
        J[2][0] += p2 * X0; J[2][1] += p2 * X1; J[2][2] += p2 * X2;
    }
    const double c11 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double c21 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double c31 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double dett = J[0][0] * c11 + J[0][1] * c21 + J[0][2] * c31;
    const double det = (__builtin_popcount(k) & 1) ? -dett : dett;  // signed det J (:1436-1442)
    const double rd = 1.0 / dett;
    const double i11 = c11 * rd, i21 = c21 * rd, i31 = c31 * rd;
    const double i12 = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * rd;
    const double i22 = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * rd;
    const double i32 = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * rd;
    const double i13 = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * rd;
    const double i23 = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * rd;
    const double i33 = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * rd;
    double P[8][3];  // dN_s/dx_c at GP k, slot j = s ^ k
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double p0 = HK_D0(j), p1 = HK_D1(j), p2 = HK_D2(j);
        P[j][0] = i11 * p0 + i12 * p1 + i13 * p2;
        P[j][1] = i21 * p0 + i22 * p1 + i23 * p2;
        P[j][2] = i31 * p0 + i32 * p1 + i33 * p2;
    }
#undef HK_D0
#undef HK_D1
#undef HK_D2
#undef HK_SG
#undef HK_MG

    // ---- volume and B-bar (cal_BVbar_hexa, :1705-1784): V = sum |det|; lane k ends up with the
    // B-bar vector of node ref_of_sign(k), the node whose force it also stores
    const double V = allreduce8(fabs(det));
    double wbar[3];
    {
        double v[8][3];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[j][c] = det * P[j][c];
        reduce_scatter8_rel(v, wbar);
    }
    const double r3V = 1.0 / (3.0 * V);
    const double bb0 = wbar[0] * r3V, bb1 = wbar[1] * r3V, bb2 = wbar[2] * r3V;
    // mean volumetric strain increment / 3 over the element
    const double* dn = nd8 + nodej[0] + 3;  // d_disp of that node
    const double sdot = allreduce8(bb0 * dn[0] + bb1 * dn[1] + bb2 * dn[2]);

    // ---- strain increment at GP k (= Bfinal * d_u, :1204)
    double Gm[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double* D = nd8 + nodej[j] + 3;
        const double d0 = D[0], d1 = D[1], d2 = D[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Gm[0][c] += d0 * P[j][c];
            Gm[1][c] += d1 * P[j][c];
            Gm[2][c] += d2 * P[j][c];
        }
    }
    constexpr double kThird = 1.0 / 3.0;
    const double vol = sdot - (Gm[0][0] + Gm[1][1] + Gm[2][2]) * kThird;
    double de[6];
    de[0] = Gm[0][0] + vol;
    de[1] = Gm[1][1] + vol;
    de[2] = Gm[2][2] + vol;
    de[3] = Gm[0][1] + Gm[1][0];
    de[4] = Gm[1][2] + Gm[2][1];
    de[5] = Gm[0][2] + Gm[2][0];

    // ---- elastic trial (:1205, :1220) and J2 radial return (:1227-1285)
    const double Dn = M->Dn, Do = M->Do, Ds = M->Ds;
    double fin[6];
    fin[0] = in.sig[0] + (Dn * de[0] + Do * (de[1] + de[2]));
    fin[1] = in.sig[1] + (Dn * de[1] + Do * (de[0] + de[2]));
    fin[2] = in.sig[2] + (Dn * de[2] + Do * (de[0] + de[1]));
    fin[3] = in.sig[3] + Ds * de[3];
    fin[4] = in.sig[4] + Ds * de[4];
    fin[5] = in.sig[5] + Ds * de[5];
    const double mean = (fin[0] + fin[1] + fin[2]) * kThird;
    double dv0 = fin[0] - mean, dv1 = fin[1] - mean, dv2 = fin[2] - mean;
    const double q =
        sqrt(1.5 * (dv0 * dv0 + dv1 * dv1 + dv2 * dv2 + 2.0 * (fin[3] * fin[3] + fin[4] * fin[4] + fin[5] * fin[5])));
    double sc = 1.0;
    if (ANY_PLASTIC && npp > 0 && q > ys) {
        const int p = plastic_segment(M->pl_eps, npp, eqp);  // (:1255-1264), 0-based
        const double H = M->Hd[p];
        const double dep = (q - ys) / (3.0 * M->G + H);
        sc = (ys + H * dep) / q;
        dv0 *= sc;
        dv1 *= sc;
        dv2 *= sc;
        fin[0] = dv0 + mean;
        fin[1] = dv1 + mean;
        fin[2] = dv2 + mean;
        fin[3] *= sc;
        fin[4] *= sc;
        fin[5] *= sc;
        eqp += dep;
        ys += H * dep;
    }
    double eps[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) eps[c] = in.eps[c] + de[c];

    // ---- triaxiality (cal_triax_stress, :995-1018): mean / Mises of the final stress. The Mises
    // of the returned stress is sc*q (radial return scales the deviator), so no second sqrt.
    const double oeq = q * sc;
    // (formed where stored, a call's last step, or where the deletion test can need it)
    double tri = STORE_TRIAX ? ((oeq < 1e-10) ? 0.0 : mean / oeq) : 0.0;
    bool kill = false;
    // a wave whose Gauss points all lie below du_skip has no element average that can reach the
    // ductile table (wave-uniform skip)
    if (DO_DELETE && nd > 0 && __builtin_amdgcn_ballot_w64(eqp >= M->du_skip) != 0) {
        const double v_e = allreduce8(eqp) * 0.125;
        if (!STORE_TRIAX) tri = (oeq < 1e-10) ? 0.0 : mean / oeq;
        const double t_e = allreduce8(tri) * 0.125;
        if (!(t_e < 0.0) && v_e >= M->du_floor)  // (below du_floor no table value is reached)
            kill = active && v_e >= ductile_fr(M->du_eps, M->du_tri, nd, t_e);  // ductile table (:720-733)
    }

    // ---- internal force (Qe[:,e] += detJ * Bfinal' * sigma, :1330-1340), reduce-scattered so
    // lane k writes the 3 components of node ref_of_sign(k).
    double fk[3];
    {
        const double w00 = det * dv0, w11 = det * dv1, w22 = det * dv2;
        const double w01 = det * fin[3], w12 = det * fin[4], w02 = det * fin[5];
        double v[8][3];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double px = P[i][0], py = P[i][1], pz = P[i][2];
            v[i][0] = w00 * px + w01 * py + w02 * pz;
            v[i][1] = w01 * px + w11 * py + w12 * pz;
            v[i][2] = w02 * px + w12 * py + w22 * pz;
        }
        reduce_scatter8_rel(v, fk);
    }
    const double S = allreduce8(det * (3.0 * mean));
    fk[0] += S * bb0;
    fk[1] += S * bb1;
    fk[2] += S * bb2;
    if (WITH_VOL) a.vol[e] = V;
    elem_writeback<DO_DELETE, STORE_TRIAX, ANY_PLASTIC, NT, false, OWN>(a, e, k, in, active, kill, fk, fin, eps, eqp,
                                                                         ys, tri, sfe);
}

}  // namespace hk
