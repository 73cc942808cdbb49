// contact_plan_check.cpp -- CPU check of the contact-model planner (test infrastructure; the planner
// is host code without HIP, csrc/hakai_contact_plan.cpp, and this program is built from it and the
// oracle's contact file oracle/hakai_oracle_contact.c alone: no GPU, no product library).
//
// Each case builds small lattice blocks of hex8 elements, plans the contact model and builds the
// oracle's contact object (literal mode, then indexed mode), then walks a deletion sequence. Before
// the first deletion and after each, for every pair: the plan's live i-nodes (orig, or an adder
// deleted -- the device's live()) equal the oracle's nodes_i as a set, likewise nodes_j, and the
// live triangles equal the oracle's (tri, tri_ele) as a multiset of (n0, n1, n2, element). Once per
// plan: pair order and instances, min/max element size bit for bit, the initial counts, the
// element -> entry CSRs against their aptr/add lists, the tiles against the regions; at every point
// of the sequence a `dup` segment against the segment whose alias serves it. Cases with several
// instances are also planned per rank for contiguous element ranges: the ranks' kept entries must be
// the one-rank plan's entries of the nodes each owns / the elements each holds, in order, adders
// included, with ni_per_rank equal to the kept i-lists. Four argument errors must return their message.
//
//   contact_plan_check              every case, one JSON line with the totals ("cases": how many ran)
//   contact_plan_check --case NAME  one case;  --list  the case names
//   contact_plan_check --lattice px py pz ix iy iz --ranks R
//                                   plate + impactor (hakai.mesh.two_body_model's shape): indexed oracle only
// JSON: {"ok", "cases", "plans", "checks", mismatch counts by kind, "digest"}; digest: 64-bit FNV-1a over
// every uploaded array of every plan of the run (PairParam without its padding word). Exit 0 iff ok.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../hakai-fem_amd/csrc/hakai_contact_plan.hpp"
#include "../oracle/hakai_oracle.h"

namespace {

using hkc::ContactPlan;
using hkc::NodeEntries;
typedef std::vector<int> ivec;

struct Fnv {
    unsigned long long h = 14695981039346656037ull;
    template <class T>
    void add(const T& v) {
        unsigned char b[sizeof(T)];
        std::memcpy(b, &v, sizeof(T));
        for (unsigned char x : b) h = (h ^ x) * 1099511628211ull;
    }
    template <class T>
    void add(const std::vector<T>& v) {
        for (const T& x : v) add(x);
    }
};

struct Mesh {
    std::vector<double> X;
    ivec conn;                  // 0-based
    std::vector<int64_t> inst;  // 1-based instance of each element
    int nN() const { return (int)X.size() / 3; }
    int nE() const { return (int)inst.size(); }
    // a lattice block of nx x ny x nz elements (element id x-fastest, C3D8 node order) with its own nodes
    void block(int nx, int ny, int nz, double ox, double oy, double oz, int instance, double h = 1.0) {
        const int n0 = nN();
        for (int z = 0; z <= nz; ++z)
            for (int y = 0; y <= ny; ++y)
                for (int x = 0; x <= nx; ++x) X.insert(X.end(), {ox + h * x, oy + h * y, oz + h * z});
        auto id = [&](int x, int y, int z) { return n0 + x + (nx + 1) * (y + (ny + 1) * z); };
        for (int z = 0; z < nz; ++z)
            for (int y = 0; y < ny; ++y)
                for (int x = 0; x < nx; ++x) {
                    conn.insert(conn.end(), {id(x, y, z), id(x + 1, y, z), id(x + 1, y + 1, z), id(x, y + 1, z),
                                             id(x, y, z + 1), id(x + 1, y, z + 1), id(x + 1, y + 1, z + 1),
                                             id(x, y + 1, z + 1)});
                    inst.push_back(instance);
                }
    }
};

struct Case {
    std::string name;
    Mesh m;
    ivec flags{1};
    std::vector<ivec> orders;  // deletion sequences (0-based elements)
    std::vector<int32_t> cp_instance;  // *Contact Pair surfaces, or none
    std::vector<int64_t> cp_off, cp_elems;
    std::vector<std::vector<int64_t>> splits;  // rank_elem_off of each multi-rank plan
    bool literal = true;
};

struct Tally {
    long long plans = 0, checks = 0, pairs = 0, sizes = 0, counts = 0, nodes_i = 0, nodes_j = 0, tri = 0, csr = 0,
              tiles = 0, dup = 0, own = 0, errors = 0;
    Fnv dg;
    long long bad() const { return pairs + sizes + counts + nodes_i + nodes_j + tri + csr + tiles + dup + own + errors; }
};

const std::vector<double> kYoung = {210e3, 70e3};

std::string plan_of(const Case& c, int flag, const hkc::ContactOwnership* own, ContactPlan& P, Tally& T) {
    ivec mat(c.m.nE());
    for (int e = 0; e < c.m.nE(); ++e) mat[e] = (int)(c.m.inst[e] - 1) % 2;
    hkc::ContactInput in;
    in.nN = c.m.nN(), in.nE = c.m.nE(), in.coord = &c.m.X, in.conn = &c.m.conn, in.mat = &mat, in.young = &kYoung;
    in.contact_flag = flag, in.element_instance = c.m.inst.data(), in.n_cp = (int)c.cp_instance.size() / 2;
    in.cp_instance = c.cp_instance.data(), in.cp_elem_off = c.cp_off.data(), in.cp_elems = c.cp_elems.data();
    in.own = own;
    const std::string err = hkc::contact_plan(in, P);
    if (!err.empty()) return err;
    ++T.plans;
    for (const hkc::PairParam& p : P.par)
        T.dg.add(p.young), T.dg.add(p.kc), T.dg.add(p.Cr), T.dg.add(p.ddiv), T.dg.add(p.self), T.dg.add(p.hash_off),
            T.dg.add(p.hash_size);
    T.dg.add(P.seg);
    for (const NodeEntries* v : {&P.ni, &P.nj}) T.dg.add(v->pair), T.dg.add(v->node), T.dg.add(v->orig), T.dg.add(v->aptr), T.dg.add(v->add);
    T.dg.add(P.tri_pair), T.dg.add(P.tri_nodes), T.dg.add(P.tri_ele), T.dg.add(P.tri_adder);
    T.dg.add(P.reg_first), T.dg.add(P.reg), T.dg.add(P.pair_reg);
    T.dg.add(P.el_ni_ptr), T.dg.add(P.el_ni), T.dg.add(P.el_nj_ptr), T.dg.add(P.el_nj), T.dg.add(P.el_tri_ptr), T.dg.add(P.el_tri);
    T.dg.add(P.tiles);
    return err;
}

bool node_live(const NodeEntries& v, int k, const std::vector<char>& del) {
    if (v.orig[k] == 1) return true;
    for (int a = v.aptr[k]; a < v.aptr[k + 1]; ++a)
        if (del[v.add[a]]) return true;
    return false;
}

// (element, entry) pairs of a CSR against those of the entries' adder lists
long long csr_bad(const ivec& ptr, const ivec& idx, const ivec& aptr, const ivec& add, int nE) {
    std::vector<std::pair<int, int>> a, b;
    if ((int)ptr.size() != nE + 1 || ptr[0] != 0 || ptr[nE] != (int)idx.size()) return 1;
    for (int e = 0; e < nE; ++e)
        for (int q = ptr[e]; q < ptr[e + 1]; ++q) a.push_back({e, idx[q]});
    for (int k = 0; k + 1 < (int)aptr.size(); ++k)
        for (int q = aptr[k]; q < aptr[k + 1]; ++q) {
            if (q > aptr[k] && add[q] <= add[q - 1]) return 1;  // an adder listed twice would expose its entry twice
            b.push_back({add[q], k});
        }
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    return a == b ? 0 : 1;
}

// once per plan: CSRs, tiles and regions
void check_structure(const ContactPlan& P, int nE, Tally& T) {
    const int n_tri = (int)P.tri_ele.size();
    T.csr += csr_bad(P.el_ni_ptr, P.el_ni, P.ni.aptr, P.ni.add, nE);
    T.csr += csr_bad(P.el_nj_ptr, P.el_nj, P.nj.aptr, P.nj.add, nE);
    ivec taptr{0}, tadd;
    for (int j = 0; j < n_tri; ++j) {
        if (P.tri_adder[j] >= 0) tadd.push_back(P.tri_adder[j]);
        taptr.push_back((int)tadd.size());
    }
    T.csr += csr_bad(P.el_tri_ptr, P.el_tri, taptr, tadd, nE);
    // every entry of every list in exactly one tile; a region's tiles are its own, in order, gapless
    const int nreg = (int)P.reg_list.size();
    std::vector<ivec> cover = {ivec(P.ni.node.size(), 0), ivec(P.nj.node.size(), 0), ivec((size_t)n_tri, 0)};
    long long bad = (int)P.reg_first.size() != nreg + 1 || (int)P.reg.size() != 2 * nreg || P.tri_reg != nreg - 1;
    ivec reg_end(nreg, 0);
    for (const hkc::Seg& s : P.seg) {
        if (s.region < 0 || s.region >= nreg - 1 || P.reg_list[s.region] != s.side || P.reg[2 * s.region] != s.start ||
            P.pair_reg[2 * s.pair + s.side] != s.region)
            ++bad;
        else
            reg_end[s.region] = s.end;
    }
    if (!bad) {
        reg_end[nreg - 1] = n_tri;
        bad += P.reg_list[nreg - 1] != 2 || P.reg[2 * (nreg - 1)] != 0 || P.reg_first[nreg] != (int)P.tiles.size();
        for (int r = 0; r < nreg && !bad; ++r) {
            int at = P.reg[2 * r];
            bad += P.reg[2 * r + 1] != 0;
            for (int t = P.reg_first[r]; t < P.reg_first[r + 1]; ++t) {
                const hkc::Tile& tl = P.tiles[t];
                if (tl.region != r || tl.list != P.reg_list[r] || tl.start != at || tl.end <= tl.start ||
                    tl.end - tl.start > hkc::kTile || tl.end > reg_end[r]) {
                    ++bad;
                    break;
                }
                for (int k = tl.start; k < tl.end; ++k) cover[tl.list][k]++;
                at = tl.end;
            }
            bad += at != reg_end[r];
        }
        for (const ivec& cv : cover)
            for (int v : cv) bad += v != 1;
    }
    T.tiles += bad ? 1 : 0;
    T.checks += 4;
}

// a dup segment has the live node set of the one segment whose alias names it
void check_dup(const ContactPlan& P, const std::vector<char>& del, Tally& T) {
    auto live_set = [&](const hkc::Seg& s) {
        const NodeEntries& v = s.side ? P.nj : P.ni;
        ivec out;
        for (int k = s.start; k < s.end; ++k)
            if (node_live(v, k, del)) out.push_back(v.node[k]);
        std::sort(out.begin(), out.end());
        return out;
    };
    for (const hkc::Seg& q : P.seg) {
        int served = 0;
        for (const hkc::Seg& r : P.seg)
            for (int al : r.alias)
                if (al == 12 * q.pair + 6 * q.side) {
                    ++served;
                    if (r.dup || live_set(r) != live_set(q)) ++T.dup;
                }
        if (served != (q.dup ? 1 : 0)) ++T.dup;
        ++T.checks;
    }
}

// the plan's live lists of every pair against the oracle's
void check_live(const ContactPlan& P, const hko_contact* O, const std::vector<char>& del, Tally& T) {
    const int np = (int)P.par.size();
    for (int p = 0; p < np; ++p) {
        int64_t info[4];
        const int64_t nj = hko_contact_pair_info(O, p, info);
        std::vector<int64_t> oi((size_t)info[2]), oj((size_t)nj), ot(3 * (size_t)info[3]), oe((size_t)info[3]);
        hko_contact_pair_lists(O, p, oi.data(), oj.data(), ot.data(), oe.data());
        std::sort(oi.begin(), oi.end());
        std::sort(oj.begin(), oj.end());
        int side = 0;
        for (const NodeEntries* v : {&P.ni, &P.nj}) {
            std::vector<int64_t> mine;
            for (int k = 0; k < (int)v->node.size(); ++k)
                if (v->pair[k] == p && node_live(*v, k, del)) mine.push_back(v->node[k] + 1);
            std::sort(mine.begin(), mine.end());
            if (mine != (side ? oj : oi)) ++(side ? T.nodes_j : T.nodes_i);
            ++side;
        }
        std::vector<std::array<int64_t, 4>> a, b;
        for (int j = 0; j < (int)P.tri_ele.size(); ++j)
            if (P.tri_pair[j] == p && (P.tri_adder[j] < 0 || del[P.tri_adder[j]]))
                a.push_back({P.tri_nodes[3 * j] + 1, P.tri_nodes[3 * j + 1] + 1, P.tri_nodes[3 * j + 2] + 1, P.tri_ele[j] + 1});
        for (size_t j = 0; j < oe.size(); ++j) b.push_back({ot[3 * j], ot[3 * j + 1], ot[3 * j + 2], oe[j]});
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        if (a != b) ++T.tri;
        T.checks += 3;
    }
}

// one flag, one deletion order, one oracle mode
void check_against_oracle(const Case& c, int flag, const ivec& order, int indexed, const ContactPlan& P, Tally& T) {
    std::vector<int64_t> conn1(c.m.conn.begin(), c.m.conn.end()), mat1(c.m.nE());
    for (int64_t& v : conn1) ++v;
    for (int e = 0; e < c.m.nE(); ++e) mat1[e] = (c.m.inst[e] - 1) % 2 + 1;
    const hko_model_view mv{c.m.nN(), c.m.nE(), c.m.X.data(), conn1.data(), mat1.data()};
    hko_contact* O = hko_contact_create_ex(&mv, flag, c.m.inst.data(), kYoung.data(), (int32_t)c.cp_instance.size() / 2,
                                           c.cp_instance.data(), c.cp_off.data(), c.cp_elems.data(), indexed);
    const int np = hko_contact_n_pairs(O);
    if (np != (int)P.par.size()) {
        ++T.pairs;
        hko_contact_destroy(O);
        return;
    }
    for (int p = 0; p < np; ++p) {
        int64_t info[4];
        const int64_t nj = hko_contact_pair_info(O, p, info);
        if (info[0] != P.pair_inst[2 * p] || info[1] != P.pair_inst[2 * p + 1] ||
            P.par[p].self != (info[0] == info[1]) || P.par[p].young != kYoung[(info[1] - 1) % 2])
            ++T.pairs;
        if (info[2] != P.pair_counts[3 * p] || info[3] != P.pair_counts[3 * p + 1] || nj != P.pair_counts[3 * p + 2]) ++T.counts;
    }
    const double mn = hko_contact_min_size(O), mx = hko_contact_max_size(O);
    if (std::memcmp(&mn, &P.min_size, 8) || std::memcmp(&mx, &P.max_size, 8)) ++T.sizes;
    T.checks += 2 * np + 1;
    std::vector<char> del((size_t)c.m.nE(), 0);
    check_live(P, O, del, T);
    check_dup(P, del, T);
    for (int e : order) {
        hko_contact_element_deleted(O, c.m.inst.data(), e + 1);
        del[e] = 1;
        check_live(P, O, del, T);
        check_dup(P, del, T);
    }
    hko_contact_destroy(O);
}

// the ranks' plans against the one-rank plan P1 (the ownership rule)
void check_split(const Case& c, int flag, const std::vector<int64_t>& off, const ContactPlan& P1, Tally& T) {
    const int nr = (int)off.size() - 1, nN = c.m.nN(), nE = c.m.nE();
    ivec owner((size_t)nN, -1), erank((size_t)nE, 0);
    for (int e = nE - 1; e >= 0; --e) {  // descending: the lowest incident element wins
        while (erank[e] < nr - 1 && e >= off[erank[e] + 1]) ++erank[e];
        for (int i = 0; i < 8; ++i) owner[c.m.conn[8 * (size_t)e + i]] = erank[e];
    }
    std::vector<ContactPlan> R((size_t)nr);
    std::vector<ivec> l2g((size_t)nr);
    for (int q = 0; q < nr; ++q) {
        ivec g2l((size_t)nN, -1);  // the rank's model: the nodes of its elements, ascending
        for (int64_t e = off[q]; e < off[q + 1]; ++e)
            for (int i = 0; i < 8; ++i) g2l[c.m.conn[8 * (size_t)e + i]] = 0;
        for (int n = 0; n < nN; ++n)
            if (g2l[n] == 0) {
                g2l[n] = (int)l2g[q].size();
                l2g[q].push_back(n);
            }
        hkc::ContactOwnership own;
        own.rank = q, own.nranks = nr, own.rank_elem_off = off.data(), own.g2l = &g2l;
        if (!plan_of(c, flag, &own, R[q], T).empty()) {
            ++T.own;
            return;
        }
        check_structure(R[q], nE, T);
        check_dup(R[q], std::vector<char>((size_t)nE, 0), T);
        check_dup(R[q], std::vector<char>((size_t)nE, 1), T);
    }
    for (int q = 0; q < nr; ++q) {
        const ContactPlan& P = R[q];
        long long bad = P.pair_inst != P1.pair_inst || P.pair_counts != P1.pair_counts || P.htot != P1.htot ||
                        std::memcmp(&P.min_size, &P1.min_size, 8) || std::memcmp(&P.max_size, &P1.max_size, 8) ||
                        std::memcmp(&P.d_lim, &P1.d_lim, 8) || (int)P.ni_per_rank.size() != nr;
        for (int r = 0; r < nr && !bad; ++r) bad += P.ni_per_rank[r] != (long long)R[r].ni.node.size();
        // node entries: P1's entries of the nodes this rank owns, in order, with their adders
        int side = 0;
        for (const NodeEntries* v1 : {&P1.ni, &P1.nj}) {
            const NodeEntries& v = side++ ? P.nj : P.ni;
            size_t k = 0;
            for (size_t k1 = 0; k1 < v1->node.size(); ++k1) {
                if (owner[v1->node[k1]] != q) continue;
                if (k >= v.node.size() || v.pair[k] != v1->pair[k1] || l2g[q][v.node[k]] != v1->node[k1] ||
                    v.orig[k] != v1->orig[k1] ||
                    ivec(v.add.begin() + v.aptr[k], v.add.begin() + v.aptr[k + 1]) !=
                        ivec(v1->add.begin() + v1->aptr[k1], v1->add.begin() + v1->aptr[k1 + 1])) {
                    ++bad;
                    break;
                }
                ++k;
            }
            bad += k != v.node.size();
        }
        // triangles: P1's triangles of this rank's elements, in order
        size_t j = 0;
        for (size_t j1 = 0; j1 < P1.tri_ele.size(); ++j1) {
            if (erank[P1.tri_ele[j1]] != q) continue;
            bool same = j < P.tri_ele.size() && P.tri_pair[j] == P1.tri_pair[j1] && P.tri_ele[j] + off[q] == P1.tri_ele[j1] &&
                        P.tri_adder[j] == P1.tri_adder[j1];
            for (int i = 0; i < 3 && same; ++i) same = l2g[q][P.tri_nodes[3 * j + i]] == P1.tri_nodes[3 * j1 + i];
            if (!same) {
                ++bad;
                break;
            }
            ++j;
        }
        bad += j != P.tri_ele.size();
        T.own += bad ? 1 : 0;
        ++T.checks;
    }
}

void run_case(const Case& c, Tally& T) {
    for (int flag : c.flags) {
        ContactPlan P;
        if (!plan_of(c, flag, nullptr, P, T).empty()) {
            ++T.errors;
            continue;
        }
        check_structure(P, c.m.nE(), T);
        for (const ivec& order : c.orders)
            for (int indexed = c.literal ? 0 : 1; indexed < 2; ++indexed) check_against_oracle(c, flag, order, indexed, P, T);
        for (const auto& off : c.splits) check_split(c, flag, off, P, T);
    }
}

// the listed elements first, then every other element ascending
ivec then_rest(ivec first, int nE) {
    for (int e = 0; e < nE; ++e)
        if (std::find(first.begin(), first.end(), e) == first.end()) first.push_back(e);
    return first;
}

std::vector<Case> all_cases() {
    std::vector<Case> cs;
    {  // single self pair; the very last face of the instance is never exterior: five of six faces
        Case c;
        c.name = "one_element";
        c.m.block(1, 1, 1, 0, 0, 0, 1);
        c.flags = {1, 2};
        c.orders = {{0}};
        cs.push_back(c);
    }
    {  // adders; nodes exposed by more than one deletion; no j-side additions of a self pair
        Case c;
        c.name = "block_self";
        c.m.block(2, 2, 2, 0, 0, 0, 1);
        c.orders = {{0, 1, 2, 3, 4, 5, 6, 7}, {7, 2, 5, 0, 3, 6, 1, 4}};
        cs.push_back(c);
    }
    {  // two directed pairs; j-side additions only when the triangle instance differs
        Case c;
        c.name = "two_blocks";
        c.m.block(3, 2, 2, 0, 0, 0, 1);
        c.m.block(2, 2, 3, 0.5, 0, 2.25, 2, 0.75);
        c.orders = {then_rest({0, 1, 4, 12, 13, 16}, 24), {23, 20, 16, 11, 7, 1}};  // corner, edge, inner-face elements
        c.splits = {{0, 12, 24}, {0, 7, 15, 24}};
        cs.push_back(c);
    }
    {  // pair enumeration order; more box duplicates than the alias table's two
        Case c;
        c.name = "three_blocks";
        c.m.block(2, 1, 1, 0, 0, 0, 1);
        c.m.block(1, 2, 1, 0, 0, 1.5, 2);
        c.m.block(1, 1, 2, 0, 0, 4, 3, 1.25);
        c.flags = {1, 2};
        c.orders = {{0, 2, 4, 1, 3, 5}};
        c.splits = {{0, 3, 6}, {0, 0, 4, 6}};
        cs.push_back(c);
    }
    {  // runs of 2 and 3 equal face keys: an odd run keeps its last face
        Case c;
        c.name = "doubled_element";
        c.m.block(2, 1, 1, 0, 0, 0, 1);
        c.m.conn.insert(c.m.conn.begin() + 8, c.m.conn.begin(), c.m.conn.begin() + 8);  // element 0 again, as element 1
        c.m.inst.push_back(1);
        c.m.block(1, 1, 1, 0, 0, 1.5, 2);
        c.flags = {1, 2};
        c.orders = {{0, 1, 2, 3}, {2, 1, 0, 3}, {1, 3, 2, 0}};
        c.splits = {{0, 1, 4}, {0, 2, 3, 4}};
        cs.push_back(c);
    }
    {  // *Contact Pair lists: the reference compares the list length only
        Case c;
        c.name = "contact_pair_lists";
        c.m.block(2, 2, 1, 0, 0, 0, 1);
        c.m.block(2, 1, 2, 0, 0, 1.5, 2);
        c.cp_instance = {1, 2, 2, 1};
        c.cp_off = {0, 2, 6, 10, 11};
        c.cp_elems = {1, 3, /* whole */ 1, 2, 3, 4, /* as long as the instance, 2 twice */ 1, 2, 2, 4, /* subset */ 2};
        c.orders = {then_rest({0, 5, 2}, 8), {7, 6, 3, 1}};
        c.splits = {{0, 4, 8}, {0, 3, 5, 8}};
        cs.push_back(c);
    }
    {  // face winding follows the sign test, not the numbering
        Case c;
        c.name = "negative_orientation";
        c.m.block(2, 1, 1, 0, 0, 0, 1);
        for (int i = 0; i < 4; ++i) std::swap(c.m.conn[i], c.m.conn[4 + i]);  // element 0: node layers swapped
        c.m.block(1, 1, 1, 0, 0, 1.5, 2);
        c.flags = {1, 2};
        c.orders = {{0, 1, 2}, {1, 0, 2}};
        c.splits = {{0, 1, 3}, {0, 1, 2, 3}};
        cs.push_back(c);
    }
    {  // a rank with no surface element (the centre of 3x3x3); a region of more than one tile
        Case c;
        c.name = "interior_rank_and_tiles";
        c.m.block(3, 3, 3, 0, 0, 0, 1);
        c.m.block(32, 32, 1, 0, 0, 3.5, 2, 0.125);
        c.orders = {{13, 4, 27, 27 + 33, 27 + 1023}};
        c.splits = {{0, 13, 1051}, {0, 13, 14, 1051}};
        cs.push_back(c);
    }
    return cs;
}

// each must return its message and build no plan
long long argument_errors(Tally& T) {
    struct E {
        std::vector<int64_t> inst;
        std::vector<int32_t> cpi;
        std::vector<int64_t> off, el;
        const char* msg;
    };
    const char* contiguous = "element_instance must number contiguous element blocks 1, 2, ...";
    const std::vector<E> es = {{{1, 3, 3}, {}, {}, {}, contiguous},
                               {{1, 2, 1}, {}, {}, {}, contiguous},
                               {{1, 1, 2}, {0, 2}, {0, 1, 2}, {1, 1}, "contact pair 1: instance 0"},
                               {{1, 1, 2}, {1, 2}, {0, 1, 2}, {3, 1}, "contact pair 1: element 3 not in instance 1"}};
    long long bad = 0;
    for (const E& e : es) {
        Case c;
        c.m.block(3, 1, 1, 0, 0, 0, 1);
        c.m.inst = e.inst;
        c.cp_instance = e.cpi, c.cp_off = e.off, c.cp_elems = e.el;
        ContactPlan P;
        const long long plans = T.plans;
        const std::string got = plan_of(c, 1, nullptr, P, T);
        if (got != e.msg || T.plans != plans || !P.par.empty() || !P.ni.node.empty() || !P.tri_ele.empty()) ++bad;
        ++T.checks;
    }
    return bad;
}

int report(const Tally& T, int cases) {
    const bool ok = T.bad() == 0 && T.plans > 0;
    std::printf("{\"ok\": %s, \"cases\": %d, \"plans\": %lld, \"checks\": %lld, \"pairs\": %lld, \"sizes\": %lld, "
                "\"counts\": %lld, \"nodes_i\": %lld, \"nodes_j\": %lld, \"tri\": %lld, \"csr\": %lld, \"tiles\": %lld, "
                "\"dup\": %lld, \"own\": %lld, \"errors\": %lld, \"digest\": \"%016llx\"}\n",
                ok ? "true" : "false", cases, T.plans, T.checks, T.pairs, T.sizes, T.counts, T.nodes_i, T.nodes_j, T.tri,
                T.csr, T.tiles, T.dup, T.own, T.errors, T.dg.h);
    return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    std::vector<Case> cs = all_cases();
    Tally T;
    if (mode == "--list") {
        for (const Case& c : cs) std::printf("%s\n", c.name.c_str());
        std::printf("argument_errors\n");
        return 0;
    }
    if (mode == "--lattice" && argc == 10 && std::string(argv[8]) == "--ranks") {
        int d[6];
        for (int i = 0; i < 6; ++i) d[i] = std::atoi(argv[2 + i]);
        const int nr = std::atoi(argv[9]);
        Case c;
        c.name = "lattice";
        c.literal = false;
        c.m.block(d[0], d[1], d[2], 0, 0, 0, 1);
        c.m.block(d[3], d[4], d[5], (d[0] - d[3]) / 2.0, (d[1] - d[4]) / 2.0, d[2] + 0.1, 2);
        const int nE = c.m.nE(), n1 = d[0] * d[1] * d[2];
        c.orders = {{n1 - 1, n1 - d[0] * d[1] / 2, n1, n1 + d[3] * d[4] / 2, 0}};
        if (nr > 1) {
            c.splits.emplace_back();
            for (int q = 0; q <= nr; ++q) c.splits[0].push_back((int64_t)nE * q / nr);
        }
        run_case(c, T);
        return report(T, 1);
    }
    if (mode == "--case" && argc == 3) {
        const std::string name = argv[2];
        if (name == "argument_errors") {
            T.errors = argument_errors(T);
            T.plans = 1;  // none is built
            return report(T, 1);
        }
        for (const Case& c : cs)
            if (c.name == name) {
                run_case(c, T);
                return report(T, 1);
            }
        std::fprintf(stderr, "no case %s\n", name.c_str());
        return 2;
    }
    if (argc != 1) {
        std::fprintf(stderr, "usage: %s [--list | --case NAME | --lattice px py pz ix iy iz --ranks R]\n", argv[0]);
        return 2;
    }
    for (const Case& c : cs) run_case(c, T);
    T.errors += argument_errors(T);
    return report(T, (int)cs.size() + 1);
}
