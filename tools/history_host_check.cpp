// history_host_check.cpp -- the host helpers of the history outputs at their edges, on the CPU
// (tests/test_history_combine_cpu.py): the combinations and CSV writers of
// hakai-fem_amd/host/hakai_history_host.cpp and hakai_elem_history_host.cpp, and the set parser and
// ring arithmetic of hakai-fem_amd/csrc/hakai_record_sets.hpp, no ROCm library. Zero records, one rank,
// 16 sets, several ranks in rank order, every refusal with the outputs left untouched, the CSV read
// back; every refusal of parse_sets and ring_check with its message, every range of small rings.
// `make _build/history_host_check_san` builds it under the host sanitizers.
//   history_host_check <scratch dir>   prints "history_host_check: OK" and returns 0, or says what failed
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../hakai-fem_amd/csrc/hakai_record_sets.hpp"
#include "../include/hakai_hip.h"

namespace hkc {
static std::string g_err;
int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace hkc

static int g_bad = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);          \
            ++g_bad;                                                    \
        }                                                               \
    } while (0)

static std::string slurp(const std::string& path) {
    std::string s;
    if (FILE* fp = std::fopen(path.c_str(), "r")) {
        char buf[4096];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof buf, fp)) > 0) s.append(buf, k);
        std::fclose(fp);
    }
    return s;
}

// values of rank r, record i, set s, field f: magnitudes spread over 2^-40 .. 2^40, so the order of
// the additions matters
static double val(int r, int64_t i, int s, int f) {
    const double scale = std::ldexp(1.0, ((r * 7 + (int)i * 3 + s * 5 + f * 11) % 81) - 40);
    return ((r + i + s + f) % 2 ? -1.0 : 1.0) * (1.0 + 0.1 * r + 0.01 * f) * scale;
}

static void combine_case(int R, int S, int64_t n) {
    const size_t W = (size_t)n * S * 16;
    std::vector<int64_t> steps((size_t)R * n), so((size_t)n, -7);
    std::vector<double> values((size_t)R * W), ke((size_t)R * S), vo(W, -7.0), ko((size_t)S, -7.0);
    for (int r = 0; r < R; ++r) {
        for (int64_t i = 0; i < n; ++i) {
            steps[(size_t)r * n + i] = 3 * i;
            for (int s = 0; s < S; ++s)
                for (int f = 0; f < 16; ++f) values[(size_t)r * W + ((size_t)i * S + s) * 16 + f] = val(r, i, s, f);
        }
        for (int s = 0; s < S; ++s) ke[(size_t)r * S + s] = val(r, 1, s, 9);
    }
    // exact-size arrays: a read or write past them is the sanitizers' to report
    CHECK(hakai_history_combine(R, S, n, n ? steps.data() : nullptr, n ? values.data() : nullptr, ke.data(),
                                n ? so.data() : nullptr, n ? vo.data() : nullptr, ko.data()) == 0);
    for (int64_t i = 0; i < n; ++i) CHECK(so[(size_t)i] == 3 * i);
    for (size_t j = 0; j < W; ++j) {
        volatile double x = values[j];
        for (int r = 1; r < R; ++r) x = x + values[(size_t)r * W + j];
        CHECK(std::memcmp(&vo[j], (const void*)&x, sizeof(double)) == 0);
    }
    for (int s = 0; s < S; ++s) {
        volatile double x = ke[(size_t)s];
        for (int r = 1; r < R; ++r) x = x + ke[(size_t)r * S + s];
        CHECK(std::memcmp(&ko[(size_t)s], (const void*)&x, sizeof(double)) == 0);
    }
    if (R == 1 && n > 0) CHECK(std::memcmp(vo.data(), values.data(), W * sizeof(double)) == 0);  // the identity
}

static void refusals() {
    int64_t steps[4] = {0, 5, 0, 6}, so[2] = {-7, -7};
    double values[64], ke[2] = {1.0, 2.0}, vo[32], ko[1] = {-7.0};
    for (int j = 0; j < 64; ++j) values[j] = 1.0 + j;
    for (int j = 0; j < 32; ++j) vo[j] = -7.0;
    auto untouched = [&] {
        bool ok = so[0] == -7 && so[1] == -7 && ko[0] == -7.0;
        for (int j = 0; j < 32; ++j) ok = ok && vo[j] == -7.0;
        return ok;
    };
    CHECK(hakai_history_combine(2, 1, 2, steps, values, ke, so, vo, ko) == HAKAI_ERR_STATE);  // steps 5 and 6
    CHECK(untouched());
    steps[3] = 5;
    CHECK(hakai_history_combine(2, 1, 2, nullptr, values, ke, so, vo, ko) == HAKAI_ERR_ARG);
    CHECK(hakai_history_combine(2, 1, 2, steps, nullptr, ke, so, vo, ko) == HAKAI_ERR_ARG);
    CHECK(hakai_history_combine(2, 1, 2, steps, values, nullptr, so, vo, ko) == HAKAI_ERR_ARG);
    CHECK(hakai_history_combine(2, 1, 2, steps, values, ke, nullptr, vo, ko) == HAKAI_ERR_ARG);
    CHECK(hakai_history_combine(2, 1, 2, steps, values, ke, so, nullptr, ko) == HAKAI_ERR_ARG);
    CHECK(hakai_history_combine(2, 1, 2, steps, values, ke, so, vo, nullptr) == HAKAI_ERR_ARG);
    CHECK(hakai_history_combine(0, 1, 2, steps, values, ke, so, vo, ko) == HAKAI_ERR_ARG);
    CHECK(hakai_history_combine(2, 0, 2, steps, values, ke, so, vo, ko) == HAKAI_ERR_ARG);
    CHECK(hakai_history_combine(2, 17, 2, steps, values, ke, so, vo, ko) == HAKAI_ERR_ARG);
    CHECK(hakai_history_combine(2, 1, -1, steps, values, ke, so, vo, ko) == HAKAI_ERR_ARG);
    CHECK(untouched());
    CHECK(hakai_history_combine(2, 1, 2, steps, values, ke, so, vo, ko) == 0);
    CHECK(so[1] == 5 && vo[0] == values[0] + values[32] && ko[0] == 3.0);
}

typedef int (*csv_fn)(const char*, int32_t, const char* const*, int64_t, const int64_t*, const double*, double);

static void csv_case(const std::string& dir, csv_fn write_csv, int F, int S, int64_t n) {
    std::vector<std::string> names;
    for (int s = 0; s < S; ++s) names.push_back(s ? "set" + std::to_string(s) : "all");
    std::vector<const char*> np;
    for (const std::string& s : names) np.push_back(s.c_str());
    std::vector<int64_t> steps((size_t)n);
    std::vector<double> values((size_t)n * S * F);
    for (int64_t i = 0; i < n; ++i) {
        steps[(size_t)i] = 10 * i;
        for (int j = 0; j < S * F; ++j) values[(size_t)i * S * F + j] = val(0, i, j / F, j % F);
    }
    const std::string path = dir + "/history_check_" + std::to_string(S) + "_" + std::to_string(n) + ".csv";
    CHECK(write_csv(path.c_str(), S, np.data(), n, n ? steps.data() : nullptr, n ? values.data() : nullptr, 1e-7) == 0);
    const std::string txt = slurp(path);
    size_t lines = 0, commas = 0;
    for (char ch : txt) {
        lines += ch == '\n';
        commas += ch == ',';
    }
    CHECK(lines == (size_t)n + 1);
    CHECK(commas == (size_t)(n + 1) * (1 + (size_t)F * S));
    // every value parses back to the same double
    size_t pos = txt.find('\n') + 1;
    for (int64_t i = 0; i < n; ++i) {
        const size_t end = txt.find('\n', pos);
        std::string line = txt.substr(pos, end - pos);
        pos = end + 1;
        char* p = &line[0];
        CHECK(std::strtoll(p, &p, 10) == steps[(size_t)i]);
        ++p;
        (void)std::strtod(p, &p);  // time
        for (int j = 0; j < S * F; ++j) {
            ++p;
            const double x = std::strtod(p, &p);
            CHECK(std::memcmp(&x, &values[(size_t)i * S * F + j], sizeof x) == 0);
        }
    }
    std::remove(path.c_str());
}

// the refusals of a CSV writer: no path, too many names, records without arrays, a directory that is not there
static void csv_refusals(const std::string& dir, csv_fn write_csv, const char* what) {
    const char* one[1] = {"all"};
    CHECK(write_csv(nullptr, 1, one, 0, nullptr, nullptr, 1.0) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == std::string(what) + ": bad arguments");
    CHECK(write_csv((dir + "/x.csv").c_str(), 17, one, 0, nullptr, nullptr, 1.0) == HAKAI_ERR_ARG);
    CHECK(write_csv((dir + "/x.csv").c_str(), 1, one, 1, nullptr, nullptr, 1.0) == HAKAI_ERR_ARG);
    CHECK(write_csv((dir + "/no/such/dir/x.csv").c_str(), 1, one, 0, nullptr, nullptr, 1.0) == HAKAI_ERR_IO);
}

// ---- the element-set history's combination: fields 0..18 add in rank order, 19 and 21 take the larger
// value with the lower id among equals (id 0: a rank without an active element), 23 the smaller value
static double eval(int r, int64_t i, int s, int f) {
    if (f == 19 || f == 21) return (double)((r * 3 + (int)i + s + f) % 4);                    // ties between ranks
    if (f == 20 || f == 22) return (r + (int)i + s) % 5 == 0 ? 0.0 : 1.0 + (r * 5 + (int)i * 3 + s + f) % 7;
    return val(r, i, s, f);
}

static void elem_combine_case(int R, int S, int64_t n) {
    const int F = 24;
    const size_t W = (size_t)n * S * F;
    std::vector<int64_t> steps((size_t)R * n), so((size_t)n, -7);
    std::vector<double> values((size_t)R * W), vo(W, -7.0);
    for (int r = 0; r < R; ++r)
        for (int64_t i = 0; i < n; ++i) {
            steps[(size_t)r * n + i] = 3 * i;
            for (int s = 0; s < S; ++s)
                for (int f = 0; f < F; ++f) {
                    double x = eval(r, i, s, f);
                    if ((f == 19 || f == 21) && eval(r, i, s, f + 1) == 0.0) x = 0.0;  // no element: value 0
                    values[(size_t)r * W + ((size_t)i * S + s) * F + f] = x;
                }
        }
    CHECK(hakai_elem_history_combine(R, S, n, n ? steps.data() : nullptr, n ? values.data() : nullptr,
                                     n ? so.data() : nullptr, n ? vo.data() : nullptr) == 0);
    for (int64_t i = 0; i < n; ++i) CHECK(so[(size_t)i] == 3 * i);
    for (size_t j = 0; j < W; ++j) {
        const int f = (int)(j % F);
        auto at = [&](int r, size_t jj) { return values[(size_t)r * W + jj]; };
        if (f <= 18) {
            volatile double x = at(0, j);
            for (int r = 1; r < R; ++r) x = x + at(r, j);
            CHECK(std::memcmp(&vo[j], (const void*)&x, sizeof(double)) == 0);
        } else if (f == 19 || f == 21) {  // the best rank among those with an element, else rank 0's pair
            int best = -1;
            for (int r = 0; r < R; ++r)
                if (at(r, j + 1) > 0.0 && (best < 0 || at(r, j) > at(best, j) ||
                                           (at(r, j) == at(best, j) && at(r, j + 1) < at(best, j + 1))))
                    best = r;
            if (best < 0) best = 0;
            CHECK(vo[j] == at(best, j) && vo[j + 1] == at(best, j + 1));
        } else if (f == 23) {
            double x = at(0, j);
            for (int r = 1; r < R; ++r) x = at(r, j) < x ? at(r, j) : x;
            CHECK(vo[j] == x);
        }
    }
    if (R == 1 && n > 0) CHECK(std::memcmp(vo.data(), values.data(), W * sizeof(double)) == 0);  // the identity
}

static void elem_refusals() {
    int64_t steps[4] = {0, 5, 0, 6}, so[2] = {-7, -7};
    double values[96], vo[48];
    for (int j = 0; j < 96; ++j) values[j] = 1.0 + j;
    for (int j = 0; j < 48; ++j) vo[j] = -7.0;
    auto untouched = [&] {
        bool ok = so[0] == -7 && so[1] == -7;
        for (int j = 0; j < 48; ++j) ok = ok && vo[j] == -7.0;
        return ok;
    };
    CHECK(hakai_elem_history_combine(2, 1, 2, steps, values, so, vo) == HAKAI_ERR_STATE);  // steps 5 and 6
    CHECK(hkc::g_err == "elem_history_combine: record 1 is step 5 on rank 0 and step 6 on rank 1 (stride and capacity "
                        "must be the same on every rank)");
    steps[3] = 5;
    CHECK(hakai_elem_history_combine(2, 1, 2, nullptr, values, so, vo) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "elem_history_combine: null array");
    CHECK(hakai_elem_history_combine(2, 1, 2, steps, nullptr, so, vo) == HAKAI_ERR_ARG);
    CHECK(hakai_elem_history_combine(2, 1, 2, steps, values, nullptr, vo) == HAKAI_ERR_ARG);
    CHECK(hakai_elem_history_combine(2, 1, 2, steps, values, so, nullptr) == HAKAI_ERR_ARG);
    CHECK(hakai_elem_history_combine(0, 1, 2, steps, values, so, vo) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "elem_history_combine: 0 ranks, 1 sets, 2 records");
    CHECK(hakai_elem_history_combine(2, 0, 2, steps, values, so, vo) == HAKAI_ERR_ARG);
    CHECK(hakai_elem_history_combine(2, 17, 2, steps, values, so, vo) == HAKAI_ERR_ARG);
    CHECK(hakai_elem_history_combine(2, 1, -1, steps, values, so, vo) == HAKAI_ERR_ARG);
    CHECK(untouched());
    CHECK(hakai_elem_history_combine(2, 1, 0, nullptr, nullptr, nullptr, nullptr) == 0);  // no record needs no array
    CHECK(hakai_elem_history_combine(2, 1, 2, steps, values, so, vo) == 0);
    CHECK(so[1] == 5 && vo[0] == values[0] + values[48]);
}

// ---- hakai_record_sets.hpp: the set parser
static void parse_case(const char* item) {
    const std::string it = item;
    std::vector<unsigned short> mask(3, 0xffff);
    auto parse = [&](int max_sets, long long n_items, int n_sets, const int64_t* off, const int64_t* ids) {
        return hkc::parse_sets("fn", item, max_sets, n_items, n_sets, off, ids, mask);
    };
    const int64_t off2[3] = {0, 2, 3}, ids2[3] = {4, 1, 4};
    CHECK(parse(15, 5, 2, off2, ids2) == 0);
    CHECK(mask.size() == 5 && mask[0] == 1 && mask[1] == 0 && mask[2] == 0 && mask[3] == 3 && mask[4] == 0);
    CHECK(parse(15, 5, 0, nullptr, nullptr) == 0);  // zero sets: nothing is read
    CHECK(mask.size() == 5 && mask[3] == 0);
    const int64_t off_e[3] = {0, 0, 0};
    CHECK(parse(15, 5, 2, off_e, nullptr) == 0);  // empty sets with null ids
    CHECK(parse(15, 0, 2, off_e, nullptr) == 0 && mask.empty());  // no item at all
    {  // the maximum number of sets: item i in sets i..15, bit s-1 for set s
        int64_t off[16], ids[120];
        int k = 0;
        for (int s = 1; s <= 15; ++s) {
            off[s - 1] = k;
            for (int i = 1; i <= s; ++i) ids[k++] = i;
        }
        off[15] = k;
        CHECK(parse(15, 15, 15, off, ids) == 0);
        for (int i = 1; i <= 15; ++i) CHECK(mask[(size_t)i - 1] == (unsigned short)(0x7fffu & ~((1u << (i - 1)) - 1u)));
        CHECK(parse(15, 15, 16, off, ids) == HAKAI_ERR_ARG);
        CHECK(hkc::g_err == "fn: 16 sets (0..15)");
    }
    CHECK(parse(15, 5, -1, off2, ids2) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: -1 sets (0..15)");
    CHECK(parse(1, 5, 2, off2, ids2) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: 2 sets (0..1)");
    CHECK(parse(15, 5, 2, nullptr, ids2) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: null set_off");
    const int64_t off_neg[3] = {-1, 2, 3}, off_dec[3] = {0, 2, 1};
    CHECK(parse(15, 5, 2, off_neg, ids2) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: bad set_off of set 1");
    CHECK(parse(15, 5, 2, off_dec, ids2) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: bad set_off of set 2");
    CHECK(parse(15, 5, 2, off2, nullptr) == HAKAI_ERR_ARG);  // a set with members and no ids
    CHECK(hkc::g_err == "fn: bad set_off of set 1");
    const int64_t ids_lo[3] = {4, 1, 0}, ids_hi[3] = {6, 1, 4}, ids_tw[3] = {4, 4, 4};
    CHECK(parse(15, 5, 2, off2, ids_lo) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: " + it + " 0 of set 2 out of 1..5");
    CHECK(parse(15, 5, 2, off2, ids_hi) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: " + it + " 6 of set 1 out of 1..5");
    CHECK(parse(15, 5, 2, off2, ids_tw) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: " + it + " 4 twice in set 1");
    CHECK(parse(15, 5, 2, off2, ids2) == 0);  // the same item in two sets is no repeat
}

// ---- hakai_record_sets.hpp: the ring's arguments and the runs of a read
static void ring_cases() {
    CHECK(hkc::ring_check("fn", 1, 1, 16) == 0);
    CHECK(hkc::ring_check("fn", 0, 1, 16) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: stride 0, capacity 1 (both >= 1)");
    CHECK(hkc::ring_check("fn", 3, 0, 16) == HAKAI_ERR_ARG);
    CHECK(hkc::g_err == "fn: stride 3, capacity 0 (both >= 1)");
    for (int64_t W : {(int64_t)16, (int64_t)24, (int64_t)256, (int64_t)384}) {
        const int64_t most = ((int64_t)1 << 40) / (1 + W);  // the largest capacity accepted
        CHECK(hkc::ring_check("fn", 1, most, W) == 0);
        CHECK(hkc::ring_check("fn", 1, most + 1, W) == HAKAI_ERR_ARG);
        CHECK(hkc::g_err == "fn: capacity too large");
    }
    for (int64_t cap = 1; cap <= 5; ++cap)
        for (int64_t nw = 0; nw <= 12; ++nw) {
            const int64_t nh = nw < cap ? nw : cap;
            for (int64_t first = -1; first <= nw + 1; ++first)
                for (int64_t n = -1; n <= nw + 2; ++n) {
                    // in range: within what was written, and a record that is read is still held
                    bool ok = first >= 0 && n >= 0 && first + n <= nw;
                    for (int64_t i = 0; ok && i < n; ++i) ok = first + i >= nw - nh;
                    const int r = hkc::read_range_check("fn", first, n, nw, nh);
                    CHECK((r == 0) == ok && (r == 0 || r == HAKAI_ERR_ARG));
                    CHECK((r == 0) == !(first < 0 || n < 0 || first + n > nw || (n > 0 && first < nw - nh)));
                    if (!ok || n == 0) continue;
                    int64_t s0 = -1, n0 = -1;
                    hkc::ring_runs(first, n, cap, &s0, &n0);
                    CHECK(n0 >= 1 && n0 <= n && s0 >= 0 && s0 + n0 <= cap && n - n0 <= cap);
                    for (int64_t i = 0; i < n; ++i) CHECK((i < n0 ? s0 + i : i - n0) == (first + i) % cap);
                }
        }
    hkc::read_range_check("fn", 2, 3, 9, 4);
    CHECK(hkc::g_err == "fn: records [2, 5) of 9 written, the newest 4 held");
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    for (int R : {1, 2, 3, 8})
        for (int S : {1, 4, 16})
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)5}) combine_case(R, S, n);
    refusals();
    for (int R : {1, 2, 3, 8})
        for (int S : {1, 4, 16})
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)5}) elem_combine_case(R, S, n);
    elem_refusals();
    for (int S : {1, 16})
        for (int64_t n : {(int64_t)0, (int64_t)3}) {
            csv_case(dir, hakai_history_write_csv, 16, S, n);
            csv_case(dir, hakai_elem_history_write_csv, 24, S, n);
        }
    csv_refusals(dir, hakai_history_write_csv, "history_write_csv");
    csv_refusals(dir, hakai_elem_history_write_csv, "elem_history_write_csv");
    parse_case("node");
    parse_case("element");
    ring_cases();
    if (g_bad) {
        std::printf("history_host_check: %d checks FAILED\n", g_bad);
        return 1;
    }
    std::printf("history_host_check: OK\n");
    return 0;
}
