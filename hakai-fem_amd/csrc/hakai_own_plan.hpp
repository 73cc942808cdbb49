// hakai_own_plan.hpp -- planner of owner-computed assembly: pure host code, no HIP, no context.
// hakai_own.cpp own_prepare fills OwnInput and uploads the plan; tools/own_plan_check.cpp replays it on
// the CPU (tests/test_own_plan.py).
#pragma once
#include <unordered_map>
#include <utility>
#include <vector>

namespace hk {

// ---------------------------------------------------------------------------------------------
// Owner-computed assembly (tuning "own_assembly"). Block lb of the persistent element kernel walks
// a SCHEDULE: the batches at positions [bstart[lb], bstart[lb+1]) of seq, ascending in batch id.
// A node's incidences, in ascending element order (the reference's serial sum,
// v2/HAKAI_j.jl:668-675), start with a run held by one block (the head segment). That block sums
// the run in an LDS slot, starting from 0.0 exactly like the nodal gather, and stores the result
// into own_q[n] (the whole Q when the run is all of them). Every later contribution is copied
// unchanged to its own row, rows of a node consecutive in element order, and the nodal kernel
// forms ((own_q[n] + row) + row) ... -- the same additions in the same order as the gather of fe,
// so the result is bit-identical whatever the schedule. Rows are numbered by super-batch (an
// export entry carries up to 4 contributions of any nodes to consecutive rows); own_ridx lists
// each node's rows in element order. One 16-B entry per node segment piece (or exported
// contribution) per super-batch of S = 2 schedule positions (1 when 2 would need more than 512
// entries), one or two per thread (format: hakai_own_entry.hpp, kernel: hakai_own_pass.hpp
// own_pass). Slots are allocated per block over the super-batches a sum is open; a schedule needing
// more than own_slot_cap open sums in one block, or a node with > 8 incidences, does not use the mode.
//
// Template form. On a lattice mesh two super-batches that meet the section's layer pattern at the
// same phase hold the same flags, counts and lanes and differ only by a constant added to their
// node targets and to their row targets. So each super-batch gets a 16-B header {template offset,
// entry count and slot offset, tbase, rbase} (own_pack_hdr), and its entries are stored with targets
// relative to tbase (ACC: the smallest node of the pass) or rbase (EXP: its smallest row); identical
// relative lists are stored once and stay in L2. The allocator's slots would break the repetition,
// so the slot is computed: slot = node mod P, which the kernel forms without a division as
// rel + tbase mod P (the header's slot offset), less P while that is >= P, at most twice. The planner
// proves P: in a block no two sums open over overlapping super-batch intervals share node mod P, and
// every relative ACC target is < 2 P. Candidates are the powers of two from the plain plan's slot count up
// to slot_cap, then the other values from slot_cap down. Without a valid P (row bands, shuffled numbering), or when a
// list of kOwnTplMinEntries or more would not shrink to half, the plan keeps the plain form only.
//
// Schedules (own_choose picks the cheapest that fits):
//  * contiguous: block lb holds batches [lb*nb/G, (lb+1)*nb/G) -- a slender section (C3) keeps all
//    of a node layer's sums open in one block;
//  * banded: on a structured region (element ids x-fastest: the +y neighbour is id+nx, the +z one
//    id+L) a wide section (C4's 200x200 plate, C5's 100x100 bar) would keep one whole node layer
//    open (10-40 k sums > 1024 slots), so most contributions became rows. The banded schedule
//    splits each layer into bands of R element rows and gives each block one band over a run of
//    layers: a node's 8 incidences then fall in one block unless it sits on a band or run edge.
// ---------------------------------------------------------------------------------------------
struct OwnSched {
    int epb = 32;                  // elements per batch: 32 (block units) or 8 (wave units)
    std::vector<int> seq;          // [nb] batch at each position
    std::vector<long long> bstart; // [G+1]
    bool banded = false;
};

struct OwnPlan {
    int S = 2;
    std::vector<int> off, list, rp, ridx;
    long long rows = 0, ne = 0;
    int max_slots = 1;
    long long round2 = 0;  // summing passes with more than one entry per thread
    // Template form (own_templates below): an equivalent second representation of off/list, present
    // when tpl is set. The kernel then reads hdr and tlist and never off and list.
    bool tpl = false;
    int P = 0;               // running-sum slots of the template form: slot = node mod P
    std::vector<int> hdr;    // [4 nb] per schedule position (super-batch starts): own_pack_hdr
    std::vector<int> tlist;  // 4 ints per stored entry, targets relative, + the no-op entry last
    long long stored = 0;    // entries in tlist (without the no-op entry)
    long long templates = 0; // distinct passes stored
    long long passes = 0;    // super-batches (headers read per step)
    // per-step bytes the lists add beyond the element/nodal kernels' own (entries read -- in template
    // form the stored entries, which stay in L2, and one header per pass --, rows written and read
    // back, row indices): what own_choose compares between schedules
    double cost() const { return 16.0 * (double)(tpl ? stored + passes : ne) + 52.0 * (double)rows; }
};

// The template store: relative passes (4 ints per entry), each distinct one kept once.
struct OwnTplStore {
    explicit OwnTplStore(std::vector<int>& store) : tl(store) {}
    int add(const int* rel, int count);  // offset (in entries) of the stored copy of this pass
    long long distinct = 0;
private:
    std::vector<int>& tl;
    std::unordered_map<unsigned long long, std::vector<std::pair<int, int>>> seen;  // hash -> (offset, count)
};

// Everything the planner reads.
struct OwnInput {
    long long nE, nN, nEp;         // elements, nodes, elements padded to whole 32-element batches
    const std::vector<int>& conn;  // [8 nE] element nodes, 0-based
    const std::vector<int>& ptr;   // [nN+1] CSR node -> incidences
    const std::vector<int>& inc0;  // incidences 8 e + local node, ascending element order per node
    int max_inc;                   // most incidences of one node
    int band_rows;                 // tuning own_band_rows (0: planned)
    int pass_batches;              // tuning own_pass_batches (0: 2 where they fit, else 1)
    const std::vector<int>* all_rows;  // nodes whose contributions must all be rows, or null
    int slot_cap[2];               // own_slot_cap for S = 1, 2
    int templates = 1;             // tuning own_templates: derive the template form where the plan admits one
};

// Candidate schedules, cheapest plan wins (OwnPlan::cost): contiguous at the persistent grid G0,
// banded at about G0 blocks (when the mesh has a structured wide section), and, if neither fits,
// contiguous at 8 G0 (finer ranges keep fewer sums open; the blocks run in waves). Super-batches
// of 2 batches where they fit 512 entries, else 1. `only` (the CPU replay harness,
// tools/own_plan_check.cpp): 0 every schedule, 1 contiguous only, 2 banded only.
bool own_choose(const OwnInput& in, long long G0, OwnSched& best_sc, OwnPlan& best, int only = 0);

}  // namespace hk
