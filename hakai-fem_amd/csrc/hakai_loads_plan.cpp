// hakai_loads_plan.cpp -- see hakai_loads_plan.hpp.
#include "hakai_loads_plan.hpp"

#include <cmath>
#include <cstdio>

#include "hakai_loads_face.hpp"

namespace hk {

namespace {
int bad(std::string& err, const char* fmt, long long a = 0, long long b = 0) {
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, a, b);
    err = buf;
    return HAKAI_ERR_ARG;
}
}  // namespace

int loads_plan(const hakai_loads_t& L, long long nN, long long nE, const int* conn, LoadsPlan& P,
               std::string& err) {
    P = LoadsPlan();
    if (L.n_amp < 0 || L.n_cload < 0 || L.n_grav < 0 || L.n_press < 0) return bad(err, "set_loads: negative count");
    if (L.n_cload >= (1LL << 30) || L.n_press >= (1LL << 28)) return bad(err, "set_loads: too many entries");
    if ((L.n_amp > 0 && (!L.amp_n || !L.amp_off || !L.amp_time || !L.amp_value)) ||
        (L.n_cload > 0 && (!L.cload_dof || !L.cload_value || !L.cload_amp)) ||
        (L.n_grav > 0 && (!L.grav_accel || !L.grav_amp)) ||
        (L.n_press > 0 && (!L.press_elem || !L.press_face || !L.press_value || !L.press_amp)))
        return bad(err, "set_loads: null array");
    // amplitude tables, packed
    for (int a = 0; a < L.n_amp; ++a) {
        if (L.amp_n[a] < 2) return bad(err, "set_loads: amplitude table %lld has %lld rows (at least 2)", a, L.amp_n[a]);
        if (L.amp_off[a] < 0) return bad(err, "set_loads: amplitude table %lld: negative offset", a);
        if (P.amp_t.size() + (size_t)L.amp_n[a] >= (size_t)1 << 30) return bad(err, "set_loads: amplitude tables too long");
        P.amp_n.push_back(L.amp_n[a]);
        P.amp_off.push_back((int)P.amp_t.size());
        for (int j = 0; j < L.amp_n[a]; ++j) {
            const double t = L.amp_time[L.amp_off[a] + j], v = L.amp_value[L.amp_off[a] + j];
            if (!std::isfinite(t) || !std::isfinite(v))
                return bad(err, "set_loads: amplitude table %lld row %lld is not finite", a, j);
            P.amp_t.push_back(t);
            P.amp_v.push_back(v);
        }
    }
    auto amp_ok = [&](int a) { return a >= -1 && a < L.n_amp; };
    // concentrated loads
    for (long long i = 0; i < L.n_cload; ++i) {
        if (L.cload_dof[i] < 1 || L.cload_dof[i] > 3 * nN)
            return bad(err, "set_loads: cload %lld: dof %lld out of range", i, L.cload_dof[i]);
        if (!amp_ok(L.cload_amp[i])) return bad(err, "set_loads: cload %lld: amplitude %lld out of range", i, L.cload_amp[i]);
        if (!std::isfinite(L.cload_value[i])) return bad(err, "set_loads: cload %lld: value is not finite", i);
    }
    if (L.n_cload > 0) {
        P.cl_ptr.assign((size_t)nN + 1, 0);
        for (long long i = 0; i < L.n_cload; ++i) P.cl_ptr[(size_t)((L.cload_dof[i] - 1) / 3) + 1]++;
        for (long long n = 0; n < nN; ++n) P.cl_ptr[n + 1] += P.cl_ptr[n];
        std::vector<int> fill(P.cl_ptr.begin(), P.cl_ptr.end() - 1);
        P.cl_comp.resize((size_t)L.n_cload);
        P.cl_amp.resize((size_t)L.n_cload);
        P.cl_val.resize((size_t)L.n_cload);
        for (long long i = 0; i < L.n_cload; ++i) {
            const long long d = L.cload_dof[i] - 1;
            const int at = fill[d / 3]++;
            P.cl_comp[at] = (int)(d % 3);
            P.cl_amp[at] = L.cload_amp[i];
            P.cl_val[at] = L.cload_value[i];
        }
    }
    // gravity
    for (int g = 0; g < L.n_grav; ++g) {
        if (!amp_ok(L.grav_amp[g])) return bad(err, "set_loads: gravity %lld: amplitude %lld out of range", g, L.grav_amp[g]);
        for (int c = 0; c < 3; ++c) {
            if (!std::isfinite(L.grav_accel[3 * g + c])) return bad(err, "set_loads: gravity %lld: not finite", g);
            P.g_acc.push_back(L.grav_accel[3 * g + c]);
        }
        P.g_amp.push_back(L.grav_amp[g]);
    }
    // pressure
    for (long long k = 0; k < L.n_press; ++k) {
        if (L.press_elem[k] < 1 || L.press_elem[k] > nE)
            return bad(err, "set_loads: pressure %lld: element %lld out of range", k, L.press_elem[k]);
        if (L.press_face[k] < 1 || L.press_face[k] > 6)
            return bad(err, "set_loads: pressure %lld: face %lld outside 1..6", k, L.press_face[k]);
        if (!amp_ok(L.press_amp[k])) return bad(err, "set_loads: pressure %lld: amplitude %lld out of range", k, L.press_amp[k]);
        if (!std::isfinite(L.press_value[k])) return bad(err, "set_loads: pressure %lld: value is not finite", k);
    }
    if (L.n_press > 0) {
        P.pr_elem.resize((size_t)L.n_press);
        P.pr_code.resize((size_t)L.n_press);
        P.pr_amp.resize((size_t)L.n_press);
        P.pr_val.resize((size_t)L.n_press);
        P.pr_ptr.assign((size_t)nN + 1, 0);
        for (long long k = 0; k < L.n_press; ++k) {
            const int e = (int)(L.press_elem[k] - 1);
            const unsigned code = loads_face_code(L.press_face[k] - 1);
            P.pr_elem[k] = e;
            P.pr_code[k] = (int)code;
            P.pr_amp[k] = L.press_amp[k];
            P.pr_val[k] = L.press_value[k];
            for (int a = 0; a < 4; ++a) P.pr_ptr[(size_t)conn[8 * (long long)e + loads_code_node(code, a)] + 1]++;
        }
        for (long long n = 0; n < nN; ++n) P.pr_ptr[n + 1] += P.pr_ptr[n];
        std::vector<int> fill(P.pr_ptr.begin(), P.pr_ptr.end() - 1);
        P.pr_ent.resize(4 * (size_t)L.n_press);
        for (long long k = 0; k < L.n_press; ++k)
            for (int a = 0; a < 4; ++a) {
                const int n = conn[8 * (long long)P.pr_elem[k] + loads_code_node((unsigned)P.pr_code[k], a)];
                P.pr_ent[fill[n]++] = (int)(4 * k + a);
            }
    }
    return 0;
}

}  // namespace hk
