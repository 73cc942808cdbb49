// conn_plan_check -- CPU round trip of the connectivity-template planner (hakai-fem_amd/csrc/
// hakai_conn_plan.cpp, the file the library compiles): builds a hex mesh as hakai_upload_model hands
// it over (0-based, padded with all-zero elements to whole 32-element batches), plans it, decodes
// every (element, lane) the way the kernel does and compares with the input. Host code only.
//
//   conn_plan_check bar NX NY NZ [NX2 NY2 NZ2] [--perm SEED] [--shuffle SEED] [--cap N]
//       one lattice bar, or two with different strides numbered one after the other (the second
//       region starts mid-batch unless NX*NY*NZ is a multiple of 32)
//       --perm: each region's local node order is permuted (some offsets become negative)
//       --shuffle: node ids are permuted at random (no structure left: must report plain)
//   conn_plan_check distinct N [--cap C]
//       a synthetic mesh of about 4 N elements with exactly N distinct patterns and no padding
//
// Prints one JSON line: "compressed" (0/1), "patterns", "base_bits", "bytes" (predicted per launch),
// "plain_bytes", "nE", "nEp", "mismatch" (decoded entries that differ; -1 without a compressed form),
// "ok". Exit status 1 when a compressed form does not decode to the input or the stats are inconsistent.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../hakai-fem_amd/csrc/hakai_conn_plan.hpp"

namespace {

// nodes x-fastest, the usual hex8 order; `order` permutes the local nodes
void add_bar(std::vector<int>& conn, int nx, int ny, int nz, int node0, const int* order) {
    const int sx = 1, sy = nx + 1, sz = (nx + 1) * (ny + 1);
    const int d[8] = {0, sx, sx + sy, sy, sz, sz + sx, sz + sx + sy, sz + sy};
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                for (int l = 0; l < 8; ++l) conn.push_back(node0 + i * sx + j * sy + k * sz + d[order[l]]);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s bar NX NY NZ [NX2 NY2 NZ2] [--perm S] [--shuffle S] [--cap N]\n"
                             "       %s distinct N [--cap C]\n", argv[0], argv[0]);
        return 2;
    }
    const std::string mode = argv[1];
    std::vector<long long> dims;
    long long perm = -1, shuffle = -1;
    int cap = hk::kConnPatCap;
    for (int a = 2; a < argc; ++a) {
        const std::string k = argv[a];
        if (k == "--perm" && a + 1 < argc) perm = std::atoll(argv[++a]);
        else if (k == "--shuffle" && a + 1 < argc) shuffle = std::atoll(argv[++a]);
        else if (k == "--cap" && a + 1 < argc) cap = std::atoi(argv[++a]);
        else if (k.rfind("--", 0) == 0) {
            std::fprintf(stderr, "bad argument %s\n", argv[a]);
            return 2;
        } else dims.push_back(std::atoll(argv[a]));
    }
    std::vector<int> conn;
    int nN = 0;
    if (mode == "bar" && (dims.size() == 3 || dims.size() == 6)) {
        std::mt19937_64 rng((unsigned long long)(perm >= 0 ? perm : 0));
        for (size_t r = 0; r < dims.size(); r += 3) {
            const int nx = (int)dims[r], ny = (int)dims[r + 1], nz = (int)dims[r + 2];
            if (nx < 1 || ny < 1 || nz < 1 || (double)(nx + 1) * (ny + 1) * (nz + 1) > 1e9) return 2;
            int order[8];
            std::iota(order, order + 8, 0);
            if (perm >= 0) std::shuffle(order, order + 8, rng);
            add_bar(conn, nx, ny, nz, nN, order);
            nN += (nx + 1) * (ny + 1) * (nz + 1);
        }
    } else if (mode == "distinct" && dims.size() == 1 && dims[0] >= 1 && dims[0] <= 1000000) {
        const int n = (int)dims[0], nE = (4 * n + 31) / 32 * 32;
        for (int e = 0; e < nE; ++e) {  // pattern e mod n: its second offset is 1 + (e mod n)
            const int base = 3 * e;
            const int d[8] = {0, 1 + e % n, 2, 3, 5, 7, 11, 13};
            for (int l = 0; l < 8; ++l) conn.push_back(base + d[l]);
        }
        nN = 3 * nE + n + 14;
    } else {
        std::fprintf(stderr, "bad mode or dimensions\n");
        return 2;
    }
    if (shuffle >= 0) {
        std::vector<int> p((size_t)nN);
        std::iota(p.begin(), p.end(), 0);
        std::mt19937_64 rng((unsigned long long)shuffle);
        std::shuffle(p.begin(), p.end(), rng);
        for (int& v : conn) v = p[(size_t)v];
    }
    const long long nE = (long long)conn.size() / 8, nEp = (nE + 31) / 32 * 32;
    conn.resize((size_t)(8 * nEp), 0);  // padding elements: all eight nodes 0

    hk::ConnPlan pl;
    const bool ok_plan = hk::conn_plan(conn.data(), nEp, pl, cap);
    long long mismatch = -1;
    bool ok = ok_plan == pl.ok;
    if (ok_plan) {
        mismatch = 0;
        ok = ok && pl.P >= 1 && pl.P <= cap && (long long)pl.rec.size() == nEp && (long long)pl.pat.size() == 8LL * pl.P &&
             pl.bytes == 4 * nEp + 32LL * pl.P;
        if (ok)
            for (long long e = 0; e < nEp; ++e) {
                ok = ok && (long long)(pl.rec[(size_t)e] >> pl.base_bits) < pl.P;
                if (!ok) break;
                for (int k = 0; k < 8; ++k) mismatch += hk::conn_decode(pl, e, k) != conn[(size_t)(8 * e + k)];
            }
        // the patterns are distinct and each starts with offset 0
        for (int p = 0; ok && p < pl.P; ++p) {
            ok = pl.pat[8 * (size_t)p] == 0;
            for (int q = 0; ok && q < p; ++q)
                ok = !std::equal(pl.pat.begin() + 8 * p, pl.pat.begin() + 8 * p + 8, pl.pat.begin() + 8 * q);
        }
        ok = ok && mismatch == 0;
    } else {
        ok = ok && pl.P == 0 && pl.rec.empty() && pl.pat.empty() && pl.bytes == 32 * nEp;
    }
    std::printf("{\"compressed\": %d, \"patterns\": %d, \"base_bits\": %d, \"bytes\": %lld, \"plain_bytes\": %lld, "
                "\"nE\": %lld, \"nEp\": %lld, \"cap\": %d, \"mismatch\": %lld, \"ok\": %s}\n",
                ok_plan ? 1 : 0, pl.P, pl.base_bits, pl.bytes, 32 * nEp, nE, nEp, cap, mismatch, ok ? "true" : "false");
    return ok ? 0 : 1;
}
