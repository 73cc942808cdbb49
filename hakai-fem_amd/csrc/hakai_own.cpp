// hakai_own.cpp -- owner-computed assembly at run time (hakai_own.hpp): the plan of
// hakai_own_plan.cpp is uploaded, switched on and off, and handed to the kernels' arguments.
#include "hakai_own.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

#include "hakai_internal.hpp"
#include "hakai_own_plan.hpp"

namespace hkc {

static bool own_live(const hakai_ctx* c) { return c->sv.q == QSrc::Own; }

void own_free(hakai_ctx* c) {
    c->own.l = Own::Lists();
    c->own.for_g0 = -1;
    c->sv.own_dropped();
}

void own_invalidate(hakai_ctx* c) {
    c->own.l.built_g = -1;
    c->own.for_g0 = -1;
    c->sv.own_dropped();
}

OwnSums own_sums(const hakai_ctx* c) {
    const Own::Lists& l = c->own.l;
    return {l.d_q, l.d_rp, l.d_ridx, l.d_rows};
}

static bool own_upload(hakai_ctx* c, const hk::OwnSched& sc, const hk::OwnPlan& pl) {
    own_free(c);
    Own::Lists& l = c->own.l;
    const long long nN = c->nN, G = (long long)sc.bstart.size() - 1;
    std::vector<int> bst(sc.bstart.begin(), sc.bstart.end());
    hipStream_t s = c->stream;
    // the entries: the template store and the headers, or the plain list and its offsets
    if ((pl.tpl ? l.d_hdr.upload(pl.hdr, s) || l.d_list.upload(pl.tlist, s)
                : l.d_off.upload(pl.off, s) || l.d_list.upload(pl.list, s)) ||
        l.d_seq.upload(sc.seq, s) || l.d_bstart.upload(bst, s) || l.d_rp.upload(pl.rp, s) || l.d_ridx.upload(pl.ridx, s) ||
        l.d_q.alloc(3 * (size_t)nN) || l.d_rows.alloc(3 * (size_t)std::max(pl.rows, 1LL)) ||
        l.d_dump.alloc(8 * (size_t)G) ||
        hipMemsetAsync(l.d_q, 0, 3 * (size_t)nN * sizeof(double), s) ||  // nodes without elements
        hipStreamSynchronize(s)) {
        own_free(c);
        return false;
    }
    l.nop = (int)(pl.tpl ? pl.stored : pl.ne);
    l.slots = pl.tpl ? pl.P : pl.max_slots;
    l.stored = pl.tpl ? pl.stored : pl.ne;
    l.templates = pl.tpl ? pl.templates : 0;
    l.rows = pl.rows;
    l.entries = pl.ne;
    l.built_g = G;
    l.s = pl.S;
    l.round2 = pl.round2;
    l.banded = sc.banded ? 1 : 0;
    return true;
}

// Owner assembly stops being used while the previous element step's forces exist only as its
// node sums (a tuning change, a list rebuild): hand the next nodal update Q through the uploaded-Q
// buffer, the same bits (k_own_q = k_nodal's own additions). Multi-GPU ranks cannot: their next
// interface fix needs the per-contribution rows.
int own_materialize(hakai_ctx* c) {
    if (!own_live(c)) return 0;
    if (c->comm)
        return fail(HAKAI_ERR_STATE, "owner-computed assembly cannot be switched off or rebuilt on a multi-GPU rank "
                    "mid-run: upload or reset the state first");
    const OwnSums o = own_sums(c);
    HIPCHK(hk::launch_own_q(o.q, o.rp, o.ridx, o.rows, c->d_qbuf, c->nN, c->stream));
    c->sv.q_uploaded();
    return 0;
}

// Grid of the persistent kernel if owner assembly may run on this context at all, else 0.
static long long own_g0(const hakai_ctx* c) {
    if (!c->own.assembly || c->nmat > hk::kMaxLdsMats || c->nE <= 0) return 0;
    return pipe_grid(c);
}

bool own_wanted(const hakai_ctx* c) {
    const Own& o = c->own;
    const long long G0 = own_g0(c);
    if (G0 <= 0 || o.for_g0 != G0 || o.l.built_g <= 0) return false;
    // The reference-order kernel's waves drift apart within a batch more than the fused kernel's, so
    // its block waits at the pass barrier for its slowest wave; passes that load a second entry
    // inside that barrier region (wide cross-sections) make the wait long, and there the fe path is
    // faster for this kernel (C5 slab 1.12 against 1.41 ms per step, C4 2.46 against 3.25,
    // profiles/r03_wave_units_sweep.log). own_assembly 2 uses the owner sums anyway (tests); a
    // multi-GPU rank whose owner sums are live keeps them (its interface fix needs the rows).
    return !(c->elem_exact && o.l.round2 > 0 && o.assembly == 1 && !(c->comm && own_live(c)));
}

// The lists are built on first use. The grid is the persistent kernel's, or 8x that (blocks then run
// in waves) when the default ranges span so much of a wide cross-section that too many sums stay
// open in a block (hk::own_choose).
bool own_prepare(hakai_ctx* c) {
    const long long G0 = own_g0(c);
    if (G0 > 0 && c->own.for_g0 != G0) {  // not yet built (or found not to fit) for this grid
        if (own_live(c) && own_materialize(c)) return false;  // (multi-GPU: step_once reports it)
        // slots per block: what two blocks per CU leave next to the kernel's own LDS (the wider
        // passes of S = 2 leave less)
        const hk::OwnInput in{c->nE, c->nN, c->nEp, c->h_conn, c->h_ptr, c->h_inc0, c->max_inc,
                              c->own.band_rows, c->own.pass_batches, comm_dn_nodes(c),
                              {hk::own_slot_cap(c->elem_exact != 0, 1, c->nmat),
                               hk::own_slot_cap(c->elem_exact != 0, 2, c->nmat)},
                              c->own.templates};
        hk::OwnSched sc;
        hk::OwnPlan pl;
        if (!(hk::own_choose(in, G0, sc, pl) && own_upload(c, sc, pl))) {
            own_free(c);
            c->own.l.built_g = -2;
        }
        c->own.for_g0 = G0;
    }
    return own_wanted(c);
}

// Connectivity templates (hakai_conn_plan.hpp): the fused element kernel has the compressed form in
// its owner-assembly template variants only, so it is in use when the mesh has one, the tuning key is
// on, the next element step takes owner assembly with its lists in template form, and the arithmetic
// is the fused kernel's.
static bool conn_in_use(const hakai_ctx* c) {
    return c->conn_templates && c->conn_P > 0 && !c->elem_exact && own_wanted(c) && c->own.l.d_hdr.get();
}

void own_elem_args(const hakai_ctx* c, hk::ElemArgs& ea) {
    const Own::Lists& l = c->own.l;
    ea.own = l.s;
    ea.own_grid = (int)l.built_g;
    ea.own_seq = l.d_seq;
    ea.own_bstart = l.d_bstart;
    ea.own_off = l.d_off;
    ea.own_list = reinterpret_cast<const int4*>(l.d_list.get());
    ea.own_hdr = reinterpret_cast<const int4*>(l.d_hdr.get());  // null: plain form
    ea.own_nop = l.nop;
    ea.own_slots = l.slots;
    ea.own_q = l.d_q;
    ea.own_rows = l.d_rows;
    ea.own_dump = l.d_dump;
    if (conn_in_use(c)) {
        ea.conn_rec = c->d_conn_rec;
        ea.conn_bits = c->conn_bits;
    }
}

int own_tuning(hakai_ctx* c, const char* key, long long value) {
    Own& o = c->own;
    if (!std::strcmp(key, "own_assembly")) {  // owner-computed node sums in the element kernel
        if (value < 0 || value > 2) return fail(HAKAI_ERR_ARG, "own_assembly must be 0, 1 or 2");
        o.assembly = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "own_pass_batches")) {  // batches per owner summing pass (0: planned)
        if (value < 0 || value > 2) return fail(HAKAI_ERR_ARG, "own_pass_batches must be 0, 1 or 2");
        if (o.pass_batches != (int)value) o.for_g0 = -1;  // re-plan at the next step
        o.pass_batches = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "own_templates")) {  // template form of the entry lists where the plan offers one
        if (value < 0 || value > 1) return fail(HAKAI_ERR_ARG, "own_templates must be 0 or 1");
        if (o.templates != (int)value) o.for_g0 = -1;  // re-plan at the next step
        o.templates = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "own_band_rows")) {  // row-band height of the banded owner schedule (0: planned)
        if (value < 0 || value > 4096) return fail(HAKAI_ERR_ARG, "own_band_rows must be in [0, 4096]");
        if (o.band_rows != (int)value) o.for_g0 = -1;  // re-plan at the next step
        o.band_rows = (int)value;
        return 0;
    }
    if (!std::strcmp(key, "elem_exact")) {  // (about to change to value)
        if (o.for_g0 == -1) return 0;
        // the owner-assembly plan was sized for the other kernel's LDS budget (the reference-order
        // kernel leaves fewer slots): re-planned before the next step (own_prepare; one context hands
        // the last sums over through own_materialize). A multi-GPU rank whose sums are live cannot
        // re-plan mid-run (its next interface fix reads the rows): it keeps a plan that fits the
        // new kernel, else the switch is refused.
        if (!(c->comm && own_live(c))) {
            o.for_g0 = -1;
        } else if (o.l.built_g > 0 && o.l.slots > hk::own_slot_cap(value != 0, o.l.s, c->nmat)) {
            return fail(HAKAI_ERR_STATE, "elem_exact: the owner-assembly lists of this multi-GPU rank need %d LDS "
                        "slots, more than the %s kernel has; switch between calls after hakai_upload_state / "
                        "hakai_reset_state", o.l.slots, value ? "reference-order" : "fused");
        }
        return 0;
    }
    return fail(HAKAI_ERR_ARG, "unknown tuning key '%s'", key);
}

int own_stat(const hakai_ctx* c, const char* key, int64_t* value) {
    const Own::Lists& l = c->own.l;
    const bool built = l.built_g > 0;
    if (!std::strcmp(key, "own_steps")) *value = c->own.steps;
    else if (!std::strcmp(key, "own_rows")) *value = built ? l.rows : -1;
    else if (!std::strcmp(key, "own_entries")) *value = built ? l.entries : -1;
    else if (!std::strcmp(key, "own_entries_stored")) *value = built ? l.stored : -1;
    else if (!std::strcmp(key, "own_templates")) *value = built ? l.templates : 0;
    else if (!std::strcmp(key, "own_superbatch")) *value = built ? l.s : 0;
    else if (!std::strcmp(key, "own_round2")) *value = built ? l.round2 : 0;
    else if (!std::strcmp(key, "own_slots")) *value = built ? l.slots : 0;
    else if (!std::strcmp(key, "own_banded")) *value = built ? l.banded : 0;
    else if (!std::strcmp(key, "own_grid")) *value = built ? l.built_g : 0;
    else if (!std::strcmp(key, "conn_patterns")) *value = conn_in_use(c) ? c->conn_P : 0;
    else if (!std::strcmp(key, "conn_bytes")) *value = conn_in_use(c) ? c->conn_bytes : 32 * c->nEp;
    else return fail(HAKAI_ERR_ARG, "unknown stat '%s'", key);
    return 0;
}

}  // namespace hkc
