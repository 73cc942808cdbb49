// hakai_contact_plan.cpp -- see hakai_contact_plan.hpp. Compiled without FP contraction: the face
// orientation, the element sizes, d_lim and the cell sizes keep the reference's roundings.
#include "hakai_contact_plan.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace {

using hkc::ContactInput;
using hkc::ContactPlan;
using hkc::NodeEntries;
using hkc::PairParam;
using hkc::Seg;

std::string msg(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

// ---- surface extraction with the reference's semantics ------------------------------------
struct Face {
    int n[4];    // oriented (global 0-based nodes)
    int key[4];  // sorted
    int ele;     // global 0-based element
};

struct Inst {
    int e0 = -1, nE = 0;
    std::vector<Face> faces;       // 6 per element, in the reference's order
    std::vector<int> order;        // face indices sorted by (key, index)
    std::vector<int> exterior;     // exterior face indices, ascending
    std::vector<std::vector<int>> added;  // per local element: faces exposed by its deletion
    double young = 0;
};

bool key_less(const Face& a, const Face& b) {
    for (int q = 0; q < 4; ++q)
        if (a.key[q] != b.key[q]) return a.key[q] < b.key[q];
    return false;
}
bool key_eq(const Face& a, const Face& b) {
    return a.key[0] == b.key[0] && a.key[1] == b.key[1] && a.key[2] == b.key[2] && a.key[3] == b.key[3];
}

void build_instance(Inst& I, const std::vector<double>& X, const std::vector<int>& conn) {
    static const int fidx[6][4] = {{0, 1, 2, 3}, {4, 5, 6, 7}, {0, 1, 5, 4}, {1, 2, 6, 5}, {2, 3, 7, 6}, {3, 0, 4, 7}};
    const int F = 6 * I.nE;
    I.faces.resize(F);
    for (int j = 0; j < I.nE; ++j) {  // get_element_face, :1944-1992
        const int e = I.e0 + j;
        const int* el = &conn[8 * (size_t)e];
        double ctr[3] = {0, 0, 0};
        for (int a = 0; a < 8; ++a)
            for (int c = 0; c < 3; ++c) ctr[c] += X[3 * (size_t)el[a] + c];
        for (int c = 0; c < 3; ++c) ctr[c] /= 8;
        for (int k = 0; k < 6; ++k) {
            Face& f = I.faces[6 * j + k];
            for (int q = 0; q < 4; ++q) f.n[q] = el[fidx[k][q]];
            const double* x1 = &X[3 * (size_t)f.n[0]];
            const double* x2 = &X[3 * (size_t)f.n[1]];
            const double* x4 = &X[3 * (size_t)f.n[3]];
            const double v1[3] = {x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]};
            const double v2[3] = {x4[0] - x1[0], x4[1] - x1[1], x4[2] - x1[2]};
            const double nv[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2],
                                  v1[0] * v2[1] - v1[1] * v2[0]};
            const double vc[3] = {ctr[0] - x1[0], ctr[1] - x1[1], ctr[2] - x1[2]};
            if (nv[0] * vc[0] + nv[1] * vc[1] + nv[2] * vc[2] > 0.) std::swap(f.n[1], f.n[3]);
            for (int q = 0; q < 4; ++q) f.key[q] = f.n[q];
            std::sort(f.key, f.key + 4);
            f.ele = e;
        }
    }
    // faces ordered by (key, index): counting sort on the smallest node, then a stable insertion
    // sort inside each (tiny) bucket -- linear time at millions of faces
    I.order.resize(F);
    {
        int kmin = INT32_MAX, kmax = -1;
        for (const Face& f : I.faces) {
            kmin = std::min(kmin, f.key[0]);
            kmax = std::max(kmax, f.key[0]);
        }
        const int nb = F ? kmax - kmin + 1 : 0;
        std::vector<int> start((size_t)nb + 1, 0);
        for (const Face& f : I.faces) start[f.key[0] - kmin + 1]++;
        for (int b = 0; b < nb; ++b) start[b + 1] += start[b];
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int i = 0; i < F; ++i) I.order[fill[I.faces[i].key[0] - kmin]++] = i;  // ascending index per bucket
        for (int b = 0; b < nb; ++b)
            for (int q = start[b] + 1; q < start[b + 1]; ++q) {
                const int v = I.order[q];
                int r = q - 1;
                while (r >= start[b] && key_less(I.faces[v], I.faces[I.order[r]])) {
                    I.order[r + 1] = I.order[r];
                    --r;
                }
                I.order[r + 1] = v;
            }
    }
    // get_surface_triangle's scan (:2040-2084): in each run of equal keys o1<o2<..<om the scan
    // pairs (o1,o2), (o3,o4), ...; an odd run keeps its LAST face, unless that is the very last
    // face of the instance (the loop stops at nE*6-1) -- SURVEY §9 Q13.
    I.exterior.clear();
    for (int a = 0; a < F;) {
        int b = a;
        while (b < F && key_eq(I.faces[I.order[a]], I.faces[I.order[b]])) ++b;
        const int m = b - a;
        const int last = I.order[b - 1];
        if ((m & 1) && last != F - 1) I.exterior.push_back(last);
        a = b;
    }
    std::sort(I.exterior.begin(), I.exterior.end());
    // add_surface_triangle (:2167-2245): for each face of the deleted element, the FIRST face (in
    // face order) with the same key that belongs to another element
    I.added.assign(I.nE, {});
    std::vector<int> run_start(F), pos_in_order(F);
    for (int i = 0; i < F; ++i) pos_in_order[I.order[i]] = i;
    for (int a = 0; a < F;) {
        int b = a;
        while (b < F && key_eq(I.faces[I.order[a]], I.faces[I.order[b]])) ++b;
        for (int q = a; q < b; ++q) run_start[I.order[q]] = a;
        a = b;
    }
    for (int j = 0; j < I.nE; ++j)
        for (int k = 0; k < 6; ++k) {
            const int fi = 6 * j + k;
            for (int q = run_start[fi]; q < F && key_eq(I.faces[I.order[q]], I.faces[fi]); ++q) {
                const int cand = I.order[q];
                if (I.faces[cand].ele == I.e0 + j) continue;
                I.added[j].push_back(cand);
                break;
            }
        }
}

// element -> entries its deletion exposes (CSR over global element ids)
void invert(const std::vector<int>& aptr, const std::vector<int>& add, int n, int nE, std::vector<int>& ptr,
            std::vector<int>& idx) {
    ptr.assign((size_t)nE + 1, 0);
    for (int k = 0; k < n; ++k)
        for (int a = aptr[k]; a < aptr[k + 1]; ++a) ptr[add[a] + 1]++;
    for (int e = 0; e < nE; ++e) ptr[e + 1] += ptr[e];
    idx.resize((size_t)ptr[nE]);
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int k = 0; k < n; ++k)
        for (int a = aptr[k]; a < aptr[k + 1]; ++a) idx[fill[add[a]]++] = k;
}

}  // namespace

namespace hkc {

std::string contact_plan(const ContactInput& in, ContactPlan& P) {
    P = ContactPlan();
    const int nE = (int)in.nE, nN = (int)in.nN;
    const std::vector<double>& X = *in.coord;
    const std::vector<int>& conn = *in.conn;
    const ContactOwnership* own = in.own;
    // owner of a node: the rank of its lowest incident element (ranks hold ascending element ranges)
    std::vector<int> owner;
    long long E0 = 0, E1 = 0;
    if (own) {
        const int64_t* off = own->rank_elem_off;
        std::vector<int> minel((size_t)nN, INT32_MAX);
        owner.assign((size_t)nN, -1);
        for (int e = 0; e < nE; ++e)
            for (int i = 0; i < 8; ++i) {
                int& m = minel[conn[8 * (size_t)e + i]];
                m = std::min(m, e);
            }
        for (int n = 0; n < nN; ++n)
            if (minel[n] != INT32_MAX) {
                const int q = (int)(std::upper_bound(off, off + own->nranks + 1, (int64_t)minel[n]) - off) - 1;
                owner[n] = q;
                if (q == own->rank && (*own->g2l)[n] < 0)
                    return msg("set_contact_global: owned node %lld is not in the local model", (long long)n + 1);
            }
        E0 = off[own->rank];
        E1 = off[own->rank + 1];
        P.ni_per_rank.assign((size_t)own->nranks, 0);
    }
    // instances: contiguous element blocks 1, 2, ... (readInpFile numbers them this way)
    std::vector<Inst> inst;
    for (int e = 0; e < nE; ++e) {
        const long long id = in.element_instance ? in.element_instance[e] : 1;
        if (id < 1) return msg("element_instance[%d] = %lld", e + 1, id);
        if ((size_t)id > inst.size()) {
            if ((size_t)id != inst.size() + 1)
                return "element_instance must number contiguous element blocks 1, 2, ...";
            inst.emplace_back();
            inst.back().e0 = e;
            inst.back().young = (*in.young)[(*in.mat)[e]];
        } else if ((size_t)id != inst.size()) {
            return "element_instance must number contiguous element blocks 1, 2, ...";
        }
        inst.back().nE++;
    }
    const int ni = (int)inst.size();
    for (auto& I : inst) build_instance(I, X, conn);
    // pairs (:273-311) and CT entries (:332-396). With *Contact Pair surfaces the exterior faces of
    // each side are restricted to the surface's elements (get_surface_triangle's "pick up only
    // contact element", :2087-2112 -- applied only when the list is not the whole instance).
    struct CtDef {
        int a, b;                                  // a: points (i side), b: triangles (j side)
        const std::vector<char>* fa = nullptr;     // element filters (instance-local), null = all
        const std::vector<char>* fb = nullptr;
    };
    std::vector<std::vector<char>> filters;
    filters.reserve(2 * (size_t)in.n_cp);
    std::vector<std::pair<int, int>> cp;
    std::vector<std::pair<const std::vector<char>*, const std::vector<char>*>> cpf;
    if (in.n_cp > 0) {
        for (int k = 0; k < in.n_cp; ++k) {
            const std::vector<char>* f[2] = {nullptr, nullptr};
            int id[2];
            for (int s = 0; s < 2; ++s) {
                id[s] = in.cp_instance[2 * k + s] - 1;
                if (id[s] < 0 || id[s] >= ni) return msg("contact pair %d: instance %d", k + 1, id[s] + 1);
                const long long b0 = in.cp_elem_off[2 * k + s], b1 = in.cp_elem_off[2 * k + s + 1];
                std::vector<char> bm((size_t)inst[id[s]].nE, 0);
                for (long long q = b0; q < b1; ++q) {
                    const long long el = in.cp_elems[q];
                    if (el < 1 || el > inst[id[s]].nE)
                        return msg("contact pair %d: element %lld not in instance %d", k + 1, el, id[s] + 1);
                    bm[el - 1] = 1;
                }
                if (b1 - b0 != inst[id[s]].nE) {  // the reference compares the list length only (:2087)
                    filters.push_back(std::move(bm));
                    f[s] = &filters.back();
                }
            }
            cp.push_back({id[0], id[1]});
            cpf.push_back({f[0], f[1]});
        }
    } else if (ni > 1) {
        for (int i = 0; i < ni; ++i)
            for (int j = (in.contact_flag == 2 ? i : i + 1); j < ni; ++j) {
                cp.push_back({i, j});
                cpf.push_back({nullptr, nullptr});
            }
    } else {
        cp.push_back({0, 0});
        cpf.push_back({nullptr, nullptr});
    }
    std::vector<CtDef> ct;
    for (size_t k = 0; k < cp.size(); ++k) {
        ct.push_back({cp[k].first, cp[k].second, cpf[k].first, cpf[k].second});
        if (cp[k].first != cp[k].second) ct.push_back({cp[k].second, cp[k].first, cpf[k].second, cpf[k].first});
    }
    const int npairs = (int)ct.size();
    // element sizes (:404-421)
    {
        double mn = INFINITY, mx = -INFINITY;
        for (int e = 0; e < nE; ++e) {
            const int* el = &conn[8 * (size_t)e];
            const double* p1 = &X[3 * (size_t)el[0]];
            const int oth[3] = {1, 3, 4};
            for (int q = 0; q < 3; ++q) {
                const double* p = &X[3 * (size_t)el[oth[q]]];
                const double a = p1[0] - p[0], b = p1[1] - p[1], d = p1[2] - p[2];
                const double L = std::sqrt(a * a + b * b + d * d);
                mn = std::min(mn, L);
                mx = std::max(mx, L);
            }
        }
        P.min_size = mn;
        P.max_size = mx;
        P.d_lim = mn * 0.3;  // :2253
    }
    struct SegKey {
        int inst;
        const void* filt;
        int adds;
    };
    std::vector<SegKey> seg_key;
    // node list of a pair side: initial exterior nodes + nodes exposed by each element's deletion
    auto keep = [](const Inst& I, const std::vector<char>* filt, int f) {
        return !filt || (*filt)[I.faces[f].ele - I.e0];
    };
    auto node_list = [&](int pr, const Inst& I, const std::vector<char>* filt, bool with_adds, NodeEntries& v,
                         bool side_i) {
        // per node: initial (exterior) or the ascending list of elements whose deletion exposes it;
        // bucketed by node id in linear time (adders arrive in ascending element order)
        std::vector<char> orig((size_t)nN, 0), seen((size_t)nN, 0);
        for (int f : I.exterior)
            if (keep(I, filt, f))
                for (int q = 0; q < 4; ++q) orig[I.faces[f].n[q]] = seen[I.faces[f].n[q]] = 1;
        std::vector<int> cnt((size_t)nN + 1, 0), adders;
        if (with_adds) {
            for (int j = 0; j < I.nE; ++j)
                for (int f : I.added[j])
                    for (int q = 0; q < 4; ++q) {
                        const int n = I.faces[f].n[q];
                        seen[n] = 1;
                        if (!orig[n]) cnt[n + 1]++;
                    }
            for (int n = 0; n < nN; ++n) cnt[n + 1] += cnt[n];
            adders.resize((size_t)cnt[nN]);
            std::vector<int> fill(cnt.begin(), cnt.end() - 1);
            for (int j = 0; j < I.nE; ++j)
                for (int f : I.added[j])
                    for (int q = 0; q < 4; ++q) {
                        const int n = I.faces[f].n[q];
                        if (!orig[n]) adders[fill[n]++] = I.e0 + j;
                    }
        }
        long long count = 0;
        for (int n = 0; n < nN; ++n) {
            if (!seen[n]) continue;
            if (own) {
                const int q = owner[n];
                if (side_i) P.ni_per_rank[q]++;
                if (q != own->rank) {
                    count += orig[n];
                    continue;
                }
            }
            v.pair.push_back(pr);
            v.node.push_back(own ? (*own->g2l)[n] : n);
            v.orig.push_back(orig[n]);
            if (!orig[n] && with_adds) {
                int last = -1;
                for (int a = cnt[n]; a < cnt[n + 1]; ++a)
                    if (adders[a] != last) v.add.push_back(last = adders[a]);  // duplicates are adjacent
            }
            v.aptr.push_back((int)v.add.size());
            count += orig[n];
        }
        return count;
    };
    int hoff = 0;
    for (int pr = 0; pr < npairs; ++pr) {
        const int a = ct[pr].a, b = ct[pr].b;  // a: points (i), b: triangles (j)
        const bool self = a == b;
        PairParam pp;
        pp.young = inst[b].young;  // :367
        pp.self = self;
        pp.kc = self ? in.kc_s : in.kc_o;
        pp.Cr = self ? in.Cr_s : in.Cr_o;
        pp.ddiv = self ? P.max_size * 0.6 : P.max_size * 1.1;  // :2322-2325
        pp.pad = 0;
        const size_t ni0 = P.ni.node.size(), nj0 = P.nj.node.size();
        // surface update (:766-804): c_nodes_i grows for every pair whose point instance lost an
        // element; triangles and c_nodes_j grow only when the triangle instance differs
        const long long c_i = node_list(pr, inst[a], ct[pr].fa, true, P.ni, true);
        const long long c_j = node_list(pr, inst[b], ct[pr].fb, !self, P.nj, false);
        long long c_t = 0;
        // a triangle (:2140-2145) of element ele, exposed from the start (adder -1) or by the deletion
        // of adder; multi-GPU: kept by the rank of ele, with local ids
        auto add_tri = [&](const int* n, int ele, int adder) {
            const int tv[6] = {n[0], n[1], n[2], n[2], n[3], n[0]};
            const bool mine = !own || (ele >= E0 && ele < E1);
            for (int h = 0; h < 2; ++h) {
                if (!mine) continue;
                P.tri_pair.push_back(pr);
                for (int q = 0; q < 3; ++q) P.tri_nodes.push_back(own ? (*own->g2l)[tv[3 * h + q]] : tv[3 * h + q]);
                P.tri_ele.push_back(own ? (int)(ele - E0) : ele);
                P.tri_adder.push_back(adder);
            }
        };
        for (int f : inst[b].exterior) {
            if (!keep(inst[b], ct[pr].fb, f)) continue;
            add_tri(inst[b].faces[f].n, inst[b].faces[f].ele, -1);
            c_t += 2;
        }
        if (!self)
            for (int j = 0; j < inst[b].nE; ++j)
                for (int f : inst[b].added[j]) add_tri(inst[b].faces[f].n, inst[b].faces[f].ele, inst[b].e0 + j);
        // a segment's live node set is a function of (instance, face filter, adders or not): equal
        // keys, equal sets at every step, so one segment's boxes serve both
        if (P.ni.node.size() > ni0) {
            P.seg.push_back({(int)ni0, (int)P.ni.node.size(), pr, 0, -1, 0, {-1, -1}});
            seg_key.push_back({a, (const void*)ct[pr].fa, 1});
        }
        if (P.nj.node.size() > nj0) {
            P.seg.push_back({(int)nj0, (int)P.nj.node.size(), pr, 1, -1, 0, {-1, -1}});
            seg_key.push_back({b, (const void*)ct[pr].fb, self ? 0 : 1});
        }
        // sized for the initial surface; nodes exposed later share buckets (slower, same result)
        int hs = 64;
        while (hs < 2 * c_i) hs <<= 1;
        pp.hash_off = hoff;
        pp.hash_size = hs;
        hoff += hs;
        P.par.push_back(pp);
        P.pair_inst.push_back(a + 1);
        P.pair_inst.push_back(b + 1);
        P.pair_counts.push_back(c_i);
        P.pair_counts.push_back(c_t);
        P.pair_counts.push_back(c_j);
    }
    P.htot = hoff;
    const int nseg = (int)P.seg.size(), n_tri = (int)P.tri_ele.size();
    for (int q = 0; q < nseg; ++q)  // bounding-box duplicates (Seg::dup / alias)
        for (int r = 0; r < q; ++r) {
            const SegKey &x = seg_key[q], &y = seg_key[r];
            if (P.seg[r].dup || x.inst != y.inst || x.filt != y.filt || x.adds != y.adds) continue;
            int* al = P.seg[r].alias;
            const int k = al[0] < 0 ? 0 : (al[1] < 0 ? 1 : -1);
            if (k < 0) break;  // r already serves two: q computes its own
            al[k] = 12 * P.seg[q].pair + 6 * P.seg[q].side;
            P.seg[q].dup = 1;
            break;
        }
    // live-list regions: i-node segments, j-node segments, then the triangle list; tiles of
    // kTile entries inside one region each (full rebuild)
    P.pair_reg.assign(2 * (size_t)npairs, -1);
    auto add_region = [&](int list, int a0, int a1) {
        const int r = (int)P.reg_first.size();
        P.reg_first.push_back((int)P.tiles.size());
        P.reg_list.push_back(list);
        P.reg.push_back(a0);
        P.reg.push_back(0);
        for (int k = a0; k < a1; k += kTile) P.tiles.push_back({list, k, std::min(a1, k + kTile), r});
        return r;
    };
    for (int list = 0; list < 2; ++list)
        for (Seg& sg : P.seg)
            if (sg.side == list) {
                sg.region = add_region(list, sg.start, sg.end);
                P.pair_reg[2 * (size_t)sg.pair + list] = sg.region;
            }
    P.tri_reg = add_region(2, 0, n_tri);
    P.reg_first.push_back((int)P.tiles.size());
    invert(P.ni.aptr, P.ni.add, (int)P.ni.node.size(), nE, P.el_ni_ptr, P.el_ni);
    invert(P.nj.aptr, P.nj.add, (int)P.nj.node.size(), nE, P.el_nj_ptr, P.el_nj);
    {
        std::vector<int> taptr((size_t)n_tri + 1, 0), tadd;
        for (int j = 0; j < n_tri; ++j) {
            if (P.tri_adder[j] >= 0) tadd.push_back(P.tri_adder[j]);
            taptr[j + 1] = (int)tadd.size();
        }
        invert(taptr, tadd, n_tri, nE, P.el_tri_ptr, P.el_tri);
    }
    return std::string();
}

}  // namespace hkc
