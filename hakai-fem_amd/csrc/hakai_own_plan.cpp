// hakai_own_plan.cpp -- planner of owner-computed assembly (hakai_own_plan.hpp).
#include "hakai_own_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <utility>

#include "hakai_own_entry.hpp"

namespace hk {

static OwnSched own_contiguous(long long nb, long long G, int epb) {
    OwnSched sc;
    sc.epb = epb;
    sc.seq.resize(nb);
    for (long long b = 0; b < nb; ++b) sc.seq[b] = (int)b;
    sc.bstart.resize(G + 1);
    for (long long lb = 0; lb <= G; ++lb) sc.bstart[lb] = lb * nb / G;
    return sc;
}

// Lattice strides of structured regions: element e's (nx, L) from a node whose 8 incidences start
// with e, {e, e+1, e+nx, e+nx+1, e+L, e+L+1, e+L+nx, e+L+nx+1}; elements without such a node (the
// last of a row, layer or region) take the previous element's. Regions = runs of equal strides.
// Returns false when the mesh shows no such lattice.
static bool lattice_strides(const OwnInput& in, std::vector<int>& nx, std::vector<int>& L) {
    const long long nE = in.nE;
    nx.assign(nE, -1);
    L.assign(nE, -1);
    long long found = 0;
    for (long long e = 0; e < nE; ++e) {
        for (int k = 0; k < 8; ++k) {
            const int n = in.conn[8 * e + k];
            const int j0 = in.ptr[n];
            if (in.ptr[n + 1] - j0 != 8 || in.inc0[j0] / 8 != e) continue;
            long long q[8];
            for (int i = 0; i < 8; ++i) q[i] = in.inc0[j0 + i] / 8 - e;
            const long long a = q[2], l = q[4];
            if (q[1] == 1 && a > 1 && q[3] == a + 1 && l > a + 1 && q[5] == l + 1 && q[6] == l + a &&
                q[7] == l + a + 1 && l % a == 0 && l < (1LL << 30)) {
                nx[e] = (int)a;
                L[e] = (int)l;
                ++found;
                break;
            }
        }
    }
    if (found * 2 < nE) return false;
    long long first = -1;
    for (long long e = 0; e < nE; ++e)
        if (nx[e] > 0) {
            first = e;
            break;
        }
    for (long long e = 0; e < nE; ++e) {
        if (nx[e] > 0) continue;
        const long long src = e < first ? first : e - 1;
        nx[e] = nx[src];
        L[e] = L[src];
    }
    return true;
}

// Banded schedule: each batch goes to the band of its first element, (region, row / R); a band's
// batches (ascending) are cut into runs, about G * (band batches) / nb of them per band.
// Band height R per region: a band of R element rows keeps up to about R + 1 node rows of sums
// open in its block -- the R - 1 interior rows of the node layer below, closing row by row while the
// layer above opens, plus what a super-batch holds (measured with tools/own_plan_check: 1071 slots
// at R = 4 on a 200-wide section, 1264 at R = 5) -- so R <= slots * 15/16 / (nx + 1) - 1. Within
// that, the exported rows per node are about 6/R at band edges plus 4 G R / (layers * rows) at run
// edges, least at R = sqrt(1.5 layers rows / G_region).
static bool own_banded(const OwnInput& in, long long G, const std::vector<int>& nx, const std::vector<int>& L,
                       int shrink, int epb, int slot_cap, OwnSched& sc) {
    const long long nb = in.nEp / epb, nE = in.nE;
    sc.epb = epb;
    // regions: contiguous id ranges of equal strides
    std::vector<long long> rstart{0};
    for (long long x = 1; x < nE; ++x)
        if (nx[x] != nx[x - 1] || L[x] != L[x - 1]) rstart.push_back(x);
    rstart.push_back(nE);
    std::vector<long long> Rreg(rstart.size() - 1);
    for (size_t r = 0; r + 1 < rstart.size(); ++r) {
        const long long e0 = rstart[r], ne = rstart[r + 1] - e0;
        const long long rows = L[e0] / nx[e0], layers = std::max<long long>(1, ne / L[e0]);
        const double Gr = std::max(1.0, (double)G * (double)ne / (double)nE);
        const long long Rcap = (slot_cap - slot_cap / 16) / (nx[e0] + 1) - 1;
        const long long Ropt = (long long)std::llround(std::sqrt(1.5 * (double)layers * (double)rows / Gr));
        const long long Rwant = in.band_rows > 0 ? (long long)in.band_rows : std::max<long long>(Ropt, 1);
        Rreg[r] = std::max<long long>(1, std::min(Rcap, Rwant) - shrink);
    }
    std::vector<long long> key(nb);
    bool any_split = false;
    size_t region = 0;
    for (long long b = 0; b < nb; ++b) {
        const long long e = std::min(epb * b, nE - 1);
        while (e >= rstart[region + 1]) ++region;
        const long long rows = L[e] / nx[e];
        long long R = Rreg[region];
        if (R >= rows) R = rows;
        else any_split = true;
        const long long row = ((e - rstart[region]) % L[e]) / nx[e];
        key[b] = ((long long)region << 32) | (row / R);
    }
    if (!any_split) return false;  // one band per layer everywhere: the contiguous schedule
    std::vector<int> order(nb);
    for (long long b = 0; b < nb; ++b) order[b] = (int)b;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key[x] < key[y]; });
    // bands: [p, q) ranges of the sorted order; runs per band apportioned to exactly G blocks in
    // total (largest remainders, at least one per band): more blocks than the persistent grid would
    // run in a second wave (a whole extra block time)
    std::vector<std::pair<long long, long long>> bands;
    for (long long p = 0; p < nb;) {
        long long q = p;
        while (q < nb && key[order[q]] == key[order[p]]) ++q;
        bands.emplace_back(p, q);
        p = q;
    }
    const long long nbands = (long long)bands.size();
    if (nbands > G) return false;
    std::vector<long long> runs(nbands);
    std::vector<std::pair<double, long long>> rem;
    long long used = 0;
    for (long long i = 0; i < nbands; ++i) {
        const long long m = bands[i].second - bands[i].first;
        const double want = (double)G * (double)m / (double)nb;
        runs[i] = std::max<long long>(1, std::min<long long>(m, (long long)want));
        used += runs[i];
        rem.emplace_back(want - (double)runs[i], i);
    }
    std::sort(rem.begin(), rem.end(), [](const std::pair<double, long long>& x, const std::pair<double, long long>& y) {
        return x.first > y.first || (x.first == y.first && x.second < y.second);
    });
    for (size_t r = 0; used < G && r < rem.size(); ++r) {
        const long long i = rem[r].second;
        if (runs[i] < bands[i].second - bands[i].first) {
            ++runs[i];
            ++used;
        }
    }
    for (long long i = 0; used > G && i < nbands; ++i)  // (the minimum of one run per band overshot)
        while (runs[i] > 1 && used > G) {
            --runs[i];
            --used;
        }
    sc.seq = order;
    sc.bstart.assign(1, 0);
    for (long long i = 0; i < nbands; ++i) {
        const long long p = bands[i].first, m = bands[i].second - p;
        for (long long r = 1; r <= runs[i]; ++r) sc.bstart.push_back(p + r * m / runs[i]);
    }
    sc.banded = true;
    return true;
}

int OwnTplStore::add(const int* rel, int count) {
    unsigned long long h = 14695981039346656037ull ^ (unsigned)count;  // FNV-1a over the whole list
    for (int q = 0; q < 4 * count; ++q) h = (h ^ (unsigned)rel[q]) * 1099511628211ull;
    std::vector<std::pair<int, int>>& cands = seen[h];
    for (const std::pair<int, int>& c : cands)  // compared on a hit: equal hashes do not prove equal lists
        if (c.second == count && (count == 0 || !std::memcmp(&tl[4 * (size_t)c.first], rel, sizeof(int) * 4 * (size_t)count)))
            return c.first;
    const int toff = (int)(tl.size() / 4);
    tl.insert(tl.end(), rel, rel + 4 * (size_t)count);
    cands.emplace_back(toff, count);
    ++distinct;
    return toff;
}

static bool own_plan(const OwnInput& in, const OwnSched& sc, int S, int slot_cap, OwnPlan& pl) {
    const int epb = sc.epb, bs = 8 * epb;  // elements per batch, threads per block
    const long long nb = in.nEp / epb, nN = in.nN;
    const long long G = (long long)sc.bstart.size() - 1;
    if (G <= 0 || in.max_inc > 8 || in.ptr.size() != (size_t)nN + 1) return false;
    pl.S = S;
    struct Ent { int target, slot, flags, n; int lanes[8]; int inc[4]; };  // inc: an EXP entry's incidences
    // pos_of[b]: schedule position of batch b; block_of[b]; sb_pos[b] = position of the first batch
    // of b's super-batch (runs of S positions from each block's first), which indexes the lists
    std::vector<int> pos_of(nb), block_of(nb);
    std::vector<long long> sb_pos(nb);
    for (long long lb = 0; lb < G; ++lb)
        for (long long p = sc.bstart[lb]; p < sc.bstart[lb + 1]; ++p) {
            const int b = sc.seq[p];
            if (p > sc.bstart[lb] && b <= sc.seq[p - 1]) return false;  // ascending within a block
            pos_of[b] = (int)p;
            block_of[b] = (int)lb;
            sb_pos[b] = sc.bstart[lb] + (p - sc.bstart[lb]) / S * S;
        }
    std::vector<std::vector<Ent>> per(nb);
    std::vector<int> rp(nN + 1, 0);
    long long rows = 0;
    // open-sum intervals per block in super-batch units: (first, last, entry refs to patch the slot)
    struct Seg { long long s0, s1; int node; std::vector<std::pair<long long, int>> refs; };
    std::vector<std::vector<Seg>> segs(G);
    auto batch_of = [&](int j) { return (long long)(in.inc0[j] / 8) / epb; };
    // LDS lane of incidence j within its super-batch: (position - super-batch position) * epb +
    // element within the batch, times 8, + local node
    auto lane_of = [&](int j) {
        const long long e = in.inc0[j] / 8;
        const long long b = e / epb;
        return (int)(((pos_of[b] - sb_pos[b]) * epb + e % epb) * 8 + in.inc0[j] % 8);
    };
    // contributions of later segments: (super-batch, incidence index j); their rows are numbered
    // in super-batch order so that one entry exports up to 4 of them (any nodes) to consecutive rows
    std::vector<std::pair<long long, int>> exports;
    // multi-GPU: the nodes shared with rank-1 send their contributions one by one (hakai_comm.cpp
    // k_pack_own), so all of them are rows
    std::vector<char> all_rows(nN, 0);
    if (const std::vector<int>* dn = in.all_rows)
        for (int n : *dn) all_rows[n] = 1;
    for (long long n = 0; n < nN; ++n) {
        const int j0 = in.ptr[n], j1 = in.ptr[n + 1];
        if (j0 == j1) continue;
        if (all_rows[n]) {
            for (int j = j0; j < j1; ++j) exports.emplace_back(sb_pos[batch_of(j)], j);
            continue;
        }
        const int hb = block_of[batch_of(j0)];
        int j = j0;
        Seg sg;
        sg.s0 = -1;
        sg.node = (int)n;
        while (j < j1 && block_of[batch_of(j)] == hb) {  // the head segment, super-batch by super-batch
            const long long sb = sb_pos[batch_of(j)];
            Ent en{(int)n, 0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0}};
            while (j < j1 && sb_pos[batch_of(j)] == sb) {
                if (en.n == 8) return false;
                en.lanes[en.n++] = lane_of(j);
                ++j;
            }
            if (sg.s0 < 0) {
                sg.s0 = sb;
                en.flags |= kOwnInit;
            }
            sg.s1 = sb;
            per[sb].push_back(en);
            sg.refs.emplace_back(sb, (int)per[sb].size() - 1);
        }
        per[sg.s1][sg.refs.back().second].flags |= kOwnFin;
        if (sg.s1 > sg.s0) segs[hb].push_back(std::move(sg));
        for (; j < j1; ++j) exports.emplace_back(sb_pos[batch_of(j)], j);
    }
    // rows: grouped by super-batch (stable: node order, then element order within a node)
    std::stable_sort(exports.begin(), exports.end(),
                     [](const std::pair<long long, int>& x, const std::pair<long long, int>& y) { return x.first < y.first; });
    std::vector<int> row_of_inc(in.inc0.size(), -1);
    for (size_t q = 0; q < exports.size();) {
        const long long sb = exports[q].first;
        Ent en{0, 0, kOwnExp, 0, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0}};
        while (q < exports.size() && exports[q].first == sb && en.n < kOwnExpRows) {
            const int j = exports[q].second;
            en.inc[en.n] = j;
            en.lanes[en.n++] = lane_of(j);
            ++q;
        }
        per[sb].push_back(en);
    }
    // Row numbers, coalesced by wave: the EXP entries of a super-batch that one wave of the pass
    // takes (list positions in one 64-aligned window, a contiguous run: they follow the node
    // entries) form a group of g entries with m <= 4 g contributions in export order (node, then
    // element). Contribution q of the group goes to row base + q, dealt to entry q mod g as its
    // (q / g)-th: so the wave's k-th stores cover g consecutive rows, and a node's rows stay
    // consecutive for the nodal kernel. An entry's target is base + i, its stride g rides in the
    // unused slot field.
    for (long long b = 0; b < nb; ++b) {
        std::vector<Ent>& v = per[b];
        for (size_t p = 0; p < v.size();) {
            if (!(v[p].flags & kOwnExp)) {
                ++p;
                continue;
            }
            size_t p1 = p;
            while (p1 < v.size() && (v[p1].flags & kOwnExp) && p1 / 64 == p / 64) ++p1;
            const int g = (int)(p1 - p);
            std::vector<std::pair<int, int>> cs;  // (incidence, lane) in export order
            for (size_t i = p; i < p1; ++i)
                for (int k = 0; k < v[i].n; ++k) cs.emplace_back(v[i].inc[k], v[i].lanes[k]);
            const int m = (int)cs.size();
            for (int i = 0; i < g; ++i) {
                Ent& en = v[p + (size_t)i];
                en.target = (int)(rows + i);
                en.slot = g;
                en.n = 0;
                for (int q = i; q < m; q += g) {
                    en.inc[en.n] = cs[(size_t)q].first;
                    en.lanes[en.n++] = cs[(size_t)q].second;
                    row_of_inc[cs[(size_t)q].first] = (int)(rows + q);
                }
            }
            rows += m;
            p = p1;
        }
    }
    // per node: its rows in element order (CSR rp / ridx)
    std::vector<int>& ridx = pl.ridx;
    ridx.clear();
    ridx.reserve(exports.size());
    for (long long n = 0; n < nN; ++n) {
        rp[n] = (int)ridx.size();
        for (int j = in.ptr[n]; j < in.ptr[n + 1]; ++j)
            if (row_of_inc[j] >= 0) ridx.push_back(row_of_inc[j]);
    }
    rp[nN] = (int)ridx.size();
    if (rows > (1LL << 31) - 1) return false;
    // slots: a sum open over super-batches [s0, s1] holds its slot through s1; reuse strictly after
    int max_slots = 1;
    for (long long lb = 0; lb < G; ++lb) {
        auto& v = segs[lb];
        std::sort(v.begin(), v.end(), [](const Seg& x, const Seg& y) { return x.s0 < y.s0; });
        std::vector<std::pair<long long, int>> busy;  // (s1, slot) min-heap
        std::vector<int> free_slots;
        int next = 0;
        auto cmp = [](const std::pair<long long, int>& x, const std::pair<long long, int>& y) { return x.first > y.first; };
        for (auto& sg : v) {
            while (!busy.empty() && busy.front().first < sg.s0) {
                free_slots.push_back(busy.front().second);
                std::pop_heap(busy.begin(), busy.end(), cmp);
                busy.pop_back();
            }
            int slot;
            if (!free_slots.empty()) {
                slot = free_slots.back();
                free_slots.pop_back();
            } else {
                slot = next++;
            }
            if (slot >= slot_cap) return false;
            max_slots = std::max(max_slots, slot + 1);
            for (auto& r : sg.refs) per[r.first][r.second].slot = slot;
            busy.emplace_back(sg.s1, slot);
            std::push_heap(busy.begin(), busy.end(), cmp);
        }
    }
    std::vector<int>& off = pl.off;
    off.assign(nb + 1, 0);
    for (long long b = 0; b < nb; ++b) {
        if (per[b].size() > 2 * (size_t)bs) return false;  // two entries per thread at most (own_pass)
        pl.round2 += per[b].size() > (size_t)bs ? 1 : 0;
        off[b + 1] = off[b] + (int)per[b].size();
    }
    const long long ne = off[nb];
    std::vector<int>& list = pl.list;
    list.assign(4 * (size_t)(ne + 1), 0);
    for (long long b = 0; b < nb; ++b)
        for (size_t i = 0; i < per[b].size(); ++i) {
            const Ent& en = per[b][i];
            own_pack(en.target, en.slot, en.flags, en.n, en.lanes, &list[4 * ((size_t)off[b] + i)]);
        }
    const int no_lanes[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // padding entry: reads lane 0, stores to the dump line
    own_pack(0, 0, kOwnNop, 0, no_lanes, &list[4 * (size_t)ne]);
    pl.rp = std::move(rp);
    pl.rows = rows;
    pl.ne = ne;
    pl.max_slots = max_slots;
    // ---- template form (hakai_own_plan.hpp): the same passes with relative targets, each distinct
    // one stored once, and slot = node mod P
    pl.tpl = false;
    pl.P = 0;
    pl.hdr.clear();
    pl.tlist.clear();
    pl.stored = pl.templates = pl.passes = 0;
    if (!in.templates) return true;
    // bases, and the widest relative ACC target (2 P must exceed it: own_tpl_slot)
    std::vector<int> tbase(nb, 0), rbase(nb, 0);
    long long max_rel = 0;
    for (long long b = 0; b < nb; ++b) {
        long long t0 = -1, t1 = -1, r0 = -1;
        for (const Ent& en : per[b]) {
            if (en.flags & kOwnExp) {
                r0 = r0 < 0 ? en.target : std::min<long long>(r0, en.target);
            } else {
                t0 = t0 < 0 ? en.target : std::min<long long>(t0, en.target);
                t1 = std::max<long long>(t1, en.target);
            }
        }
        tbase[b] = (int)std::max(t0, 0LL);
        rbase[b] = (int)std::max(r0, 0LL);
        max_rel = std::max(max_rel, t1 - t0);
    }
    // P is valid when, in every block, no two sums open over overlapping super-batch intervals
    // share node mod P (segs[lb] is sorted by s0: a sum still holding the slot shows as s1 >= s0)
    std::vector<long long> until;
    auto valid = [&](int P) {
        for (long long lb = 0; lb < G; ++lb) {
            until.assign((size_t)P, -1);
            for (const Seg& sg : segs[lb]) {
                long long& u = until[(size_t)(sg.node % P)];
                if (u >= sg.s0) return false;
                u = sg.s1;
            }
        }
        return true;
    };
    int P = 0;
    {
        const long long least = std::max<long long>(max_slots, max_rel / 2 + 1);  // rel < 2 P
        long long p2 = 1;
        while (p2 < least) p2 *= 2;
        for (; p2 <= slot_cap && !P; p2 *= 2)
            if (valid((int)p2)) P = (int)p2;
        // (no power of two fits the reference-order kernel's 874 slots on a 20x20 section, whose
        // open sums span more than 512 ids; and a modulus near a multiple of the node-layer stride
        // folds two open layers onto each other, so the others are tried from the largest down --
        // a modulus that fails does so within the first blocks)
        for (long long p = slot_cap; p >= least && !P; --p)
            if (valid((int)p)) P = (int)p;
    }
    if (!P) return true;  // plain form only
    OwnTplStore store(pl.tlist);
    std::vector<int> rel;
    pl.hdr.assign(4 * (size_t)nb, 0);
    for (long long lb = 0; lb < G; ++lb)
        for (long long b = sc.bstart[lb]; b < sc.bstart[lb + 1]; b += S) {  // the super-batches' first positions
            ++pl.passes;
            const int cnt = (int)per[b].size();
            rel.resize(4 * (size_t)cnt);
            for (int i = 0; i < cnt; ++i) {
                const Ent& en = per[b][(size_t)i];
                const bool ex = (en.flags & kOwnExp) != 0;
                own_pack(en.target - (ex ? rbase[b] : tbase[b]), ex ? en.slot : 0, en.flags, en.n, en.lanes, &rel[4 * (size_t)i]);
            }
            own_pack_hdr(store.add(rel.data(), cnt), cnt, tbase[b] % P, tbase[b], rbase[b], &pl.hdr[4 * (size_t)b]);
        }
    pl.templates = store.distinct;
    std::vector<int>& tl = pl.tlist;
    pl.stored = (long long)(tl.size() / 4);
    tl.resize(tl.size() + 4);
    own_pack(0, 0, kOwnNop, 0, no_lanes, &tl[4 * (size_t)pl.stored]);
    if (pl.ne >= kOwnTplMinEntries && 2 * (pl.stored + pl.passes) > pl.ne) {  // the store would not halve the list
        pl.hdr.clear();
        pl.tlist.clear();
        pl.stored = pl.templates = 0;
        return true;
    }
    pl.P = P;
    pl.tpl = true;
    return true;
}

bool own_choose(const OwnInput& in, long long G0, OwnSched& best_sc, OwnPlan& best, int only) {
    const int epb = 32;
    const long long nb = in.nEp / epb;
    // slots per block: what two blocks per CU leave next to the kernel's own LDS (the wider
    // passes of S = 2 leave less); row bands are sized for S = 2
    auto cap_of = [&](int S) { return in.slot_cap[S - 1]; };
    const int cap = cap_of(2);
    bool have = false;
    auto consider = [&](const OwnSched& sc) {
        for (int S : {2, 1}) {
            if (in.pass_batches > 0 && S != in.pass_batches) continue;
            OwnPlan pl;
            if (!own_plan(in, sc, S, cap_of(S), pl)) continue;
            if (!have || pl.cost() < best.cost()) {
                best = std::move(pl);
                best_sc = sc;
                have = true;
            }
            return true;  // S = 2 fits: S = 1 only adds passes
        }
        return false;
    };
    if (only != 2) consider(own_contiguous(nb, G0, epb));
    if (only != 1) {
        std::vector<int> nx, L;
        if (lattice_strides(in, nx, L)) {
            OwnSched sc;
            for (int shrink : {0, 1, 2, 4})  // the widest bands whose open sums fit a block's slots
                if (own_banded(in, G0, nx, L, shrink, epb, cap, sc) && consider(sc)) break;
        }
    }
    if (!have && only != 2 && 8 * G0 <= nb) consider(own_contiguous(nb, 8 * G0, epb));
    return have;
}

}  // namespace hk
