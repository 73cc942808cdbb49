// hakai_own.hpp -- run-time state of owner-computed assembly (tuning "own_assembly"): the persistent
// element kernel sums node forces in LDS in element order and stores Q (or a prefix partial plus the
// later contributions as rows) instead of the per-element fe array. The planner is
// hakai_own_plan.cpp, the entry format hakai_own_entry.hpp; hakai_own.cpp uploads a plan and switches
// it on and off. Whether the last element step's sums are live is StepView's Q source (QSrc::Own).
#pragma once
#include "hakai_devmem.hpp"
#include "hakai_kernels.hpp"

struct hakai_ctx;

namespace hkc {

struct Own {
    int assembly = 1;        // tuning value (1 = use when eligible; env HAKAI_OWN_ASSEMBLY)
    int band_rows = 0;       // tuning: row-band height of the banded schedule (0: planned)
    int pass_batches = 0;    // tuning: batches per summing pass (0: 2 where they fit, else 1)
    int templates = 1;       // tuning: 1 = template form of the entry lists when the plan offers one
    long long for_g0 = -1;   // persistent-kernel grid the lists were built for (a change rebuilds)
    long long steps = 0;     // element steps run with owner-computed assembly
    // The uploaded plan; own_free drops it whole.
    struct Lists {
        long long built_g = -1;    // grid the lists were built for (-1 none, -2 mesh not suitable)
        DevBuf<int> d_off;         // [nb+1] entry offsets per schedule position (super-batch starts)
        DevBuf<int> d_seq;         // [nb] batch at each schedule position (ascending within a block)
        DevBuf<int> d_bstart;      // [grid+1] first schedule position of each block
        int banded = 0;            // the schedule walks row bands of a structured cross-section
        long long round2 = 0;      // summing passes that take a second entry per thread
        DevBuf<int> d_list;        // 4 ints per entry (+ one no-op entry at nop); template form: the store
        DevBuf<int> d_hdr;         // template form: [nb] 16-byte headers, indexed like d_off (then not uploaded)
        long long stored = 0;      // entries in d_list without the no-op entry (= entries in plain form)
        long long templates = 0;   // distinct passes stored (0: plain form)
        int nop = 0;
        int slots = 0;             // LDS running-sum slots the lists use (the kernel's dynamic LDS)
        DevBuf<double> d_q;        // [nN][3]
        DevBuf<int> d_rp;          // [nN+1]
        DevBuf<double> d_rows;     // [rows][3], numbered by super-batch
        DevBuf<int> d_ridx;        // rows of node n: d_ridx[d_rp[n] .. d_rp[n+1]), element order
        DevBuf<double> d_dump;     // [grid][8]
        long long rows = 0, entries = 0;
        int s = 2;                 // batches per super-batch (2, or 1)
    } l;
};

// The node sums as their readers take them (k_nodal, k_own_q, the interface kernels).
struct OwnSums {
    const double* q;
    const int* rp;
    const int* ridx;
    const double* rows;
};
OwnSums own_sums(const hakai_ctx* c);

void own_free(hakai_ctx* c);
// The interface changed (the lists export every dn node's contributions): rebuilt at the next call.
void own_invalidate(hakai_ctx* c);
// Start of a stepping call and of each step: (re)builds the lists for the current grid and tuning
// values, handing live sums over through own_materialize, never inside a graph capture (the call's
// start has done it by then). Returns own_wanted.
bool own_prepare(hakai_ctx* c);
// The next element step uses owner-computed assembly; pure, valid once own_prepare has run for the
// current grid.
bool own_wanted(const hakai_ctx* c);
// Owner assembly stops being used while the last element step's forces exist only as its node sums:
// they become the uploaded-Q buffer's content, the same bits.
int own_materialize(hakai_ctx* c);
void own_elem_args(const hakai_ctx* c, hk::ElemArgs& ea);
// The "own_*" tuning keys, and what a change of "elem_exact" to `value` means for the lists.
int own_tuning(hakai_ctx* c, const char* key, long long value);
int own_stat(const hakai_ctx* c, const char* key, int64_t* value);  // the "own_*" stats

}  // namespace hkc
