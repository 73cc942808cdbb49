// hakai_walls_plan.cpp -- see hakai_walls_plan.hpp.
#include "hakai_walls_plan.hpp"

#include <cmath>
#include <cstdio>

#include "hakai_walls_node.hpp"

namespace hk {

namespace {
int bad(std::string& err, const char* fmt, long long a = 0, long long b = 0) {
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, a, b);
    err = buf;
    return HAKAI_ERR_ARG;
}
}  // namespace

int walls_plan(const hakai_walls_t& W, long long nN, WallsPlan& P, std::string& err) {
    P = WallsPlan();
    if (W.n_amp < 0 || W.n_wall < 0) return bad(err, "set_walls: negative count");
    if (W.n_wall > HAKAI_MAX_WALLS) return bad(err, "set_walls: %lld walls (at most %lld)", W.n_wall, HAKAI_MAX_WALLS);
    if ((W.n_amp > 0 && (!W.amp_n || !W.amp_off || !W.amp_time || !W.amp_value)) ||
        (W.n_wall > 0 && (!W.origin || !W.normal || !W.motion || !W.amp || !W.stiffness || !W.scale || !W.damping ||
                          !W.friction || !W.node_off)))
        return bad(err, "set_walls: null array");
    // amplitude tables, packed
    for (int a = 0; a < W.n_amp; ++a) {
        if (W.amp_n[a] < 2) return bad(err, "set_walls: amplitude table %lld has %lld rows (at least 2)", a, W.amp_n[a]);
        if (W.amp_off[a] < 0) return bad(err, "set_walls: amplitude table %lld: negative offset", a);
        if (P.amp_t.size() + (size_t)W.amp_n[a] >= (size_t)1 << 30) return bad(err, "set_walls: amplitude tables too long");
        P.amp_n.push_back(W.amp_n[a]);
        P.amp_off.push_back((int)P.amp_t.size());
        for (int j = 0; j < W.amp_n[a]; ++j) {
            const double t = W.amp_time[W.amp_off[a] + j], v = W.amp_value[W.amp_off[a] + j];
            if (!std::isfinite(t) || !std::isfinite(v))
                return bad(err, "set_walls: amplitude table %lld row %lld is not finite", a, j);
            P.amp_t.push_back(t);
            P.amp_v.push_back(v);
        }
    }
    bool any_list = false;
    for (int w = 0; w < W.n_wall; ++w) {
        if (W.amp[w] < -1 || W.amp[w] >= W.n_amp) return bad(err, "set_walls: wall %lld: amplitude %lld out of range", w, W.amp[w]);
        double nrm[3], n[3];
        for (int c = 0; c < 3; ++c) {
            if (!std::isfinite(W.origin[3 * w + c]) || !std::isfinite(W.motion[3 * w + c]))
                return bad(err, "set_walls: wall %lld: origin or motion is not finite", w);
            if (!std::isfinite(W.normal[3 * w + c])) return bad(err, "set_walls: wall %lld: normal is not finite", w);
            nrm[c] = W.normal[3 * w + c];
        }
        const double len = walls_normalise(nrm, n);
        if (!(len > 0.0) || !std::isfinite(len))
            return bad(err, "set_walls: wall %lld: the normal's length is not finite and positive", w);
        const double par[4] = {W.stiffness[w], W.scale[w], W.damping[w], W.friction[w]};
        for (int q = 0; q < 4; ++q)
            if (!std::isfinite(par[q]) || par[q] < 0.0)
                return bad(err, "set_walls: wall %lld: stiffness, scale, damping and friction must be finite and >= 0", w);
        const long long n0 = W.node_off[w], n1 = W.node_off[w + 1];
        if (n0 < 0 || n1 < n0) return bad(err, "set_walls: wall %lld: node_off is not ascending", w);
        if (n1 > n0 && !W.nodes) return bad(err, "set_walls: null array");
        for (long long j = n0; j < n1; ++j)
            if (W.nodes[j] < 1 || W.nodes[j] > nN)
                return bad(err, "set_walls: wall %lld: node %lld out of range", w, W.nodes[j]);
        any_list = any_list || n1 > n0;
        for (int c = 0; c < 3; ++c) P.tab.push_back(n[c]);
        for (int c = 0; c < 3; ++c) P.tab.push_back(W.origin[3 * w + c]);
        for (int c = 0; c < 3; ++c) P.tab.push_back(W.motion[3 * w + c]);
        for (int q = 0; q < 4; ++q) P.tab.push_back(par[q]);
        P.amp.push_back(W.amp[w]);
    }
    P.n_wall = W.n_wall;
    if (any_list) {
        P.mask.assign((size_t)nN, 0u);
        for (int w = 0; w < W.n_wall; ++w) {
            const unsigned bit = 1u << w;
            const long long n0 = W.node_off[w], n1 = W.node_off[w + 1];
            if (n1 == n0)
                for (long long n = 0; n < nN; ++n) P.mask[(size_t)n] |= bit;
            else
                for (long long j = n0; j < n1; ++j) P.mask[(size_t)(W.nodes[j] - 1)] |= bit;  // twice counts once
        }
    }
    return 0;
}

}  // namespace hk
