// own_plan_check.cpp -- CPU replay of the owner-computed assembly plans (test infrastructure; the
// planner is host code without HIP, csrc/hakai_own_plan.cpp own_choose / own_plan, and this program
// is built from it and the entry format csrc/hakai_own_entry.hpp alone: no GPU, no product library).
//
// Builds a structured hex mesh (hakai.mesh.hex_bar numbering: element id x-fastest, C3D8 node
// order), or two of them (plate + impactor, C4's shape), optionally with shuffled element ids, runs
// the planner for one configuration and then REPLAYS the plan exactly as k_element_pipe and k_nodal
// execute it: every block walks its schedule positions, stages its super-batch's contributions by
// lane, runs the super-batch's entries (INIT/continue/FIN sums in LDS slots, exported rows), and the
// nodal side forms own_q[n] + rows in own_ridx order. The result must equal, bit for bit, the
// reference's serial assembly Q[n] = ((0 + c_1) + c_2) + ... in ascending element order
// (v2/HAKAI_j.jl:668-675) for random contributions with mixed signs and magnitudes.
//
//   own_plan_check nx ny nz [--plate px py pz] [--G n] [--exact 0|1] [--schedule 0|1|2]
//                  [--shuffle seed] [--band-rows R]
//   own_plan_check --selftest
// Prints one JSON line: {"ok": ..., "planned": ..., "epb", "grid", "superbatch", "banded", "rows",
// "entries", "slots", "mismatch", "digest"} and exits 0 when the replay matches (or no plan fits:
// planned false). digest: 64-bit FNV-1a over the plan (epb, S, seq, bstart, off, list, rp, ridx).
// Where the plan offers the template form (hakai_own_plan.hpp: headers, relative targets, slot =
// node mod P) the replay runs a second time in that form, exactly as the kernel reads it, and both
// must match; "template_form" (0 or 1), "templates" (distinct passes), "entries_stored", "passes"
// and "template_slots" (P) report it.
// --selftest packs entries and headers at the field extremes and reads them back, checks node mod P
// by conditional subtraction, and that the template store keeps two passes apart that differ in one
// lane id (exit 1 on a mismatch).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../hakai-fem_amd/csrc/hakai_kernels.hpp"  // own_slot_cap only (host code, no HIP call)
#include "../hakai-fem_amd/csrc/hakai_own_entry.hpp"
#include "../hakai-fem_amd/csrc/hakai_own_plan.hpp"

namespace {

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

// Pack and re-read entries at the extremes of every field, with and without the kernel's kOwnRound2.
int selftest() {
    long long bad = 0, n_checked = 0;
    for (int slot : {0, 1023, 1024, hk::kOwnSlotsMax - 1})
        for (int n = 0; n <= 8; ++n)
            for (int flags : {0, (int)hk::kOwnInit, (int)hk::kOwnFin, (int)hk::kOwnExp, (int)hk::kOwnNop})
                for (int pos = 0; pos <= 8; ++pos)  // 8: every lane at the base value
                    for (int base : {0, 511}) {
                        int lanes[8], w[4];
                        for (int j = 0; j < 8; ++j) lanes[j] = j == pos ? 511 - base : base;
                        const int target = (n_checked & 1) ? INT_MAX : (int)(n_checked % 1000);
                        hk::own_pack(target, slot, flags, n, lanes, w);
                        bool ok = w[0] == target && !(w[1] & hk::kOwnRound2);
                        for (int y : {w[1], w[1] | hk::kOwnRound2}) {
                            ok = ok && hk::own_slot(y) == slot && hk::own_flags(y) == flags && hk::own_n(y) == n;
                            for (int j = 0; j < 8; ++j) ok = ok && hk::own_lane(y, w[2], w[3], j) == lanes[j];
                        }
                        bad += ok ? 0 : 1;
                        ++n_checked;
                    }
    // header fields at their extremes, and node mod P without a division
    for (int count : {0, 1, 512})
        for (int sofs : {0, 1, hk::kOwnSlotsMax - 1}) {
            int h[4];
            hk::own_pack_hdr(INT_MAX, count, sofs, INT_MAX - 1, 7, h);
            bad += (h[0] == INT_MAX && hk::own_hdr_count(h[1]) == count && hk::own_hdr_sofs(h[1]) == sofs &&
                    h[2] == INT_MAX - 1 && h[3] == 7) ? 0 : 1;
            ++n_checked;
        }
    for (int P : {1, 2, 874, 1024, hk::kOwnSlotsMax})
        for (int tbase : {0, 1, P - 1, P, 12345, INT_MAX - hk::kOwnSlotsMax})
            for (int rel : {0, 1, P / 2, P - 1, P, 2 * P - 1}) {
                bad += hk::own_tpl_slot(rel, tbase % P, P) == (int)(((long long)tbase + rel) % P) ? 0 : 1;
                ++n_checked;
            }
    // the template store: two passes that differ in one lane id only do not share a template; equal
    // ones do; a pass that is a prefix of another does not
    {
        std::vector<int> tl;
        hk::OwnTplStore store(tl);
        int a[8], b[8], la[8] = {1, 2, 3, 4, 5, 6, 7, 8}, lb[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        hk::own_pack(0, 0, hk::kOwnInit, 8, la, a);
        hk::own_pack(5, 0, hk::kOwnInit | hk::kOwnFin, 8, la, a + 4);
        lb[7] = 9;  // the lane kept in y
        hk::own_pack(0, 0, hk::kOwnInit, 8, la, b);
        hk::own_pack(5, 0, hk::kOwnInit | hk::kOwnFin, 8, lb, b + 4);
        const int oa = store.add(a, 2), ob = store.add(b, 2), oa2 = store.add(a, 2), o1 = store.add(a, 1);
        lb[7] = 8, lb[3] = 0;  // a lane kept in z | w
        hk::own_pack(5, 0, hk::kOwnInit | hk::kOwnFin, 8, lb, b + 4);
        const int oc = store.add(b, 2);
        bad += (oa == 0 && ob == 2 && oa2 == oa && o1 == 4 && oc == 5 && store.distinct == 4 && tl.size() == 4 * 7) ? 0 : 1;
        ++n_checked;
    }
    std::printf("{\"ok\": %s, \"selftest\": %lld, \"bad\": %lld}\n", bad ? "false" : "true", n_checked, bad);
    return bad ? 1 : 0;
}

void hex_bar(int nx, int ny, int nz, int node0, std::vector<int>& conn) {
    auto id = [&](int x, int y, int z) { return node0 + x + (nx + 1) * (y + (ny + 1) * z); };
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int v[8] = {id(x, y, z),         id(x + 1, y, z),         id(x + 1, y + 1, z),
                                  id(x, y + 1, z),     id(x, y, z + 1),         id(x + 1, y, z + 1),
                                  id(x + 1, y + 1, z + 1), id(x, y + 1, z + 1)};
                conn.insert(conn.end(), v, v + 8);
            }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "--selftest") return selftest();
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s nx ny nz [--plate px py pz] [--G n] [--exact e] [--schedule s] "
                     "[--shuffle seed] [--band-rows R]\n       %s --selftest\n", argv[0], argv[0]);
        return 2;
    }
    const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]), nz = std::atoi(argv[3]);
    int px = 0, py = 0, pz = 0, exact = 0, schedule = 0, band_rows = 0;
    long long G0 = 512;
    long long shuffle = -1;
    for (int a = 4; a < argc; ++a) {
        const std::string k = argv[a];
        if (k == "--plate" && a + 3 < argc) {
            px = std::atoi(argv[++a]);
            py = std::atoi(argv[++a]);
            pz = std::atoi(argv[++a]);
        } else if (k == "--G" && a + 1 < argc) G0 = std::atoll(argv[++a]);
        else if (k == "--exact" && a + 1 < argc) exact = std::atoi(argv[++a]);
        else if (k == "--schedule" && a + 1 < argc) schedule = std::atoi(argv[++a]);
        else if (k == "--shuffle" && a + 1 < argc) shuffle = std::atoll(argv[++a]);
        else if (k == "--band-rows" && a + 1 < argc) band_rows = std::atoi(argv[++a]);
        else {
            std::fprintf(stderr, "bad argument %s\n", argv[a]);
            return 2;
        }
    }
    // mesh: [plate] then the bar (two instances, like hakai.mesh.two_body_model)
    std::vector<int> conn;
    int nN = 0;
    if (px > 0) {
        hex_bar(px, py, pz, 0, conn);
        nN = (px + 1) * (py + 1) * (pz + 1);
    }
    hex_bar(nx, ny, nz, nN, conn);
    nN += (nx + 1) * (ny + 1) * (nz + 1);
    long long nE = (long long)conn.size() / 8;
    if (shuffle >= 0) {  // random element numbering
        std::vector<int> perm(nE);
        for (long long e = 0; e < nE; ++e) perm[e] = (int)e;
        std::mt19937_64 rng((unsigned long long)shuffle);
        std::shuffle(perm.begin(), perm.end(), rng);
        std::vector<int> c2(conn.size());
        for (long long e = 0; e < nE; ++e)
            for (int k = 0; k < 8; ++k) c2[8 * e + k] = conn[8 * (size_t)perm[e] + k];
        conn.swap(c2);
    }
    const long long nEp = (nE + 31) / 32 * 32;
    // node -> (8e + k) CSR in ascending element order (hakai_upload_model)
    std::vector<int> cnt(nN + 1, 0);
    for (long long e = 0; e < nE; ++e)
        for (int k = 0; k < 8; ++k) ++cnt[conn[8 * e + k] + 1];
    int maxinc = 0;
    for (int n = 0; n < nN; ++n) maxinc = std::max(maxinc, cnt[n + 1]);
    for (int n = 0; n < nN; ++n) cnt[n + 1] += cnt[n];
    const std::vector<int>& ptr = cnt;
    std::vector<int> inc0(8 * (size_t)nE, 0);
    std::vector<int> fill(cnt.begin(), cnt.end() - 1);
    for (long long e = 0; e < nE; ++e)
        for (int k = 0; k < 8; ++k) inc0[fill[conn[8 * e + k]]++] = (int)(8 * e + k);
    const hk::OwnInput in{nE, nN, nEp, conn, ptr, inc0, maxinc, band_rows, /*pass_batches*/ 0, /*all_rows*/ nullptr,
                          {hk::own_slot_cap(exact != 0, 1, 1), hk::own_slot_cap(exact != 0, 2, 1)}};
    const long long G = std::min<long long>(G0, nEp / 32);

    hk::OwnSched sc;
    hk::OwnPlan pl;
    const bool planned = hk::own_choose(in, G, sc, pl, schedule);
    if (!planned) {
        std::printf("{\"ok\": true, \"planned\": false, \"elements\": %lld, \"nodes\": %d}\n", nE, nN);
        return 0;
    }
    // ---- replay (one force component is enough: the three are summed alike)
    const int epb = sc.epb, S = pl.S;
    const long long Gp = (long long)sc.bstart.size() - 1;
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> mag(-30.0, 30.0);
    std::vector<double> f(8 * (size_t)nEp, 0.0);
    for (long long e = 0; e < nE; ++e)
        for (int k = 0; k < 8; ++k) {
            const double m = std::ldexp(1.0, (int)mag(rng));
            f[8 * e + k] = (rng() & 1 ? -1.0 : 1.0) * m * (1.0 + (double)(rng() >> 11) * 0x1p-53);
        }
    auto lane_of = [](const int* w, int j) { return hk::own_lane(w[1], w[2], w[3], j); };
    long long bad = 0, mismatch = 0;
    // tpl: the template form, executed as the kernel does -- the super-batch's header, then its stored
    // entries with the bases added and the slot derived (hakai_own_entry.hpp own_tpl_slot)
    auto replay = [&](bool tpl) {
        std::vector<double> own_q(nN, 0.0), rows(std::max<long long>(pl.rows, 1), 0.0);
        std::vector<char> q_set(nN, 0);
        std::vector<double> slots(4096, 0.0);
        std::vector<double> stage(8 * (size_t)epb * S);
        for (long long lb = 0; lb < Gp; ++lb) {
            for (long long p0 = sc.bstart[lb]; p0 < sc.bstart[lb + 1]; p0 += S) {
                const long long p1 = std::min<long long>(p0 + S, sc.bstart[lb + 1]);
                std::fill(stage.begin(), stage.end(), 0.0);
                for (long long p = p0; p < p1; ++p)
                    for (int l = 0; l < 8 * epb; ++l) {
                        const long long e = (long long)sc.seq[p] * epb + l / 8;
                        stage[(p - p0) * 8 * epb + l] = e < nE ? f[8 * e + l % 8] : 0.0;
                    }
                const int* h = tpl ? &pl.hdr[4 * (size_t)p0] : nullptr;
                const int q0 = tpl ? h[0] : pl.off[p0], q1 = tpl ? h[0] + hk::own_hdr_count(h[1]) : pl.off[p0 + 1];
                if (tpl && q1 > pl.stored) ++bad;
                for (int q = q0; q < q1; ++q) {
                    const int* w = tpl ? &pl.tlist[4 * (size_t)q] : &pl.list[4 * (size_t)q];
                    const int flags = hk::own_flags(w[1]), n = hk::own_n(w[1]);
                    const bool exp = (flags & hk::kOwnExp) != 0;
                    const long long target = tpl ? (long long)w[0] + (exp ? h[3] : h[2]) : w[0];
                    int slot = hk::own_slot(w[1]);
                    if (tpl && !exp) {
                        slot = hk::own_tpl_slot(w[0], hk::own_hdr_sofs(h[1]), pl.P);
                        if (slot < 0 || slot >= pl.P || slot != (int)(target % pl.P)) ++bad;
                    }
                    if (exp) {
                        for (int j = 0; j < n; ++j) rows[target + (long long)j * slot] = stage[lane_of(w, j)];
                        continue;
                    }
                    if (flags & hk::kOwnNop) continue;
                    double v = (flags & hk::kOwnInit) ? 0.0 : slots[slot];
                    for (int j = 0; j < n; ++j) v += stage[lane_of(w, j)];
                    if (flags & hk::kOwnFin) {
                        if (q_set[target]) ++bad;  // a node's sum is finished once
                        q_set[target] = 1;
                        own_q[target] = v;
                    } else {
                        slots[slot] = v;
                    }
                }
            }
        }
        for (int n = 0; n < nN; ++n) {
            double ref = 0.0;
            for (int j = ptr[n]; j < ptr[n + 1]; ++j) ref += f[inc0[j]];
            double q = own_q[n];
            for (int r = pl.rp[n]; r < pl.rp[n + 1]; ++r) q += rows[pl.ridx[r]];
            if (std::memcmp(&q, &ref, sizeof q) != 0) ++mismatch;
        }
    };
    replay(false);
    if (pl.tpl) replay(true);
    const bool ok = mismatch == 0 && bad == 0;
    Fnv dg;
    dg.add(epb), dg.add(S), dg.add(sc.seq), dg.add(sc.bstart), dg.add(pl.off), dg.add(pl.list), dg.add(pl.rp), dg.add(pl.ridx);
    std::printf("{\"ok\": %s, \"planned\": true, \"elements\": %lld, \"nodes\": %d, \"epb\": %d, \"grid\": %lld, "
                "\"superbatch\": %d, \"banded\": %d, \"rows\": %lld, \"entries\": %lld, \"slots\": %d, "
                "\"slot_cap\": %d, \"round2\": %lld, \"mismatch\": %lld, \"double_fin\": %lld, \"digest\": \"%016llx\", "
                "\"template_form\": %d, \"templates\": %lld, \"entries_stored\": %lld, \"passes\": %lld, "
                "\"template_slots\": %d}\n",
                ok ? "true" : "false", nE, nN, epb, Gp, S, sc.banded ? 1 : 0, pl.rows, pl.ne, pl.max_slots,
                in.slot_cap[S - 1], pl.round2, mismatch, bad, dg.h, pl.tpl ? 1 : 0, pl.templates,
                pl.tpl ? pl.stored : pl.ne, pl.passes, pl.P);
    return ok ? 0 : 1;
}
