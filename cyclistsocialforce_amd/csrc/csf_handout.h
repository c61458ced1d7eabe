// csf_handout.h — the order in which a workgroup of pair_cull_kernel hands its receivers to its waves (csf_pair.hip: COMPACT).
//
// A visit - one receiver against one tile - sifts the receiver's candidate batches two at a time; how many passes that takes is
// known from the batch masks before the visit starts.  Handing the long visits out first keeps a wave from claiming a long
// one when its siblings are about to leave (list scheduling, longest job first).  Which wave takes a receiver, and when,
// enters no sum: a receiver's visit is one wave's, and its noted corrections are added by that wave, in the order they were noted.
//
// Device and host share the weight and its classes; handout_ranks is the host's copy of the ranking the kernel forms with
// ballots (tests/test_handout_rank.py through csf_handout_ranks).
#pragma once
#include <stdint.h>

namespace csf {

// sift passes at their price in vector instructions per source (profiles/pair_plain_f32_isa_counts.txt: 48 with both batches
// inside the field of view, 64 with its exact test), in units of 16
constexpr unsigned HANDOUT_W_IN = 3, HANDOUT_W_FOV = 4;
// a receiver's class: 0 (handed out first) weight >= T0, 1 >= T1, 2 >= T2, 3 the rest.  Geometric: within a class two visits
// differ by less than a factor two, and the order within a class is the receivers' own
constexpr unsigned HANDOUT_T0 = 32, HANDOUT_T1 = 16, HANDOUT_T2 = 8;

// cand / inside: the visit's candidate batches and those of them wholly inside the field of view (both masked to the tile's
// batches).  Inside batches go through the sift in pairs, an odd one joins the partial batches.
__host__ __device__ inline unsigned handout_weight(unsigned cand, unsigned inside) {
    const unsigned ni = (unsigned)__builtin_popcount(inside);
    const unsigned np = (unsigned)__builtin_popcount(cand & ~inside) + (ni & 1u);
    return HANDOUT_W_IN * (ni >> 1) + HANDOUT_W_FOV * ((np + 1u) >> 1);
}

// Host copy of the kernel's ranking.  rank[r] for every receiver r < n whose candidate mask is not empty ("wanted"): a
// permutation of 0 .. n_wanted - 1, by class, then by index; -1 for the others.  Returns n_wanted.
inline int handout_ranks(const uint32_t *cand, const uint32_t *inside, int n, int32_t *rank) {
    // (step by step what the kernel does: lane r holds receiver r, a ballot is a mask over the lanes, mbcnt the set bits below a lane)
    uint64_t wanted = 0, ge0 = 0, ge1 = 0, ge2 = 0;
    unsigned w[64];
    for (int r = 0; r < n && r < 64; r++) {
        w[r] = handout_weight(cand[r], inside[r] & cand[r]);
        wanted |= (uint64_t)(cand[r] != 0u) << r;
        ge0 |= (uint64_t)(w[r] >= HANDOUT_T0) << r, ge1 |= (uint64_t)(w[r] >= HANDOUT_T1) << r, ge2 |= (uint64_t)(w[r] >= HANDOUT_T2) << r;
    }
    const uint64_t m0 = ge0 & wanted, m1 = ge1 & ~ge0 & wanted, m2 = ge2 & ~ge1 & wanted, m3 = wanted & ~ge2;
    const int n0 = __builtin_popcountll(m0), n1 = n0 + __builtin_popcountll(m1), n2 = n1 + __builtin_popcountll(m2);
    for (int r = 0; r < n && r < 64; r++) {
        const uint64_t lower = (1ull << r) - 1ull;
        int k = n2 + __builtin_popcountll(m3 & lower);
        k = w[r] >= HANDOUT_T2 ? n1 + __builtin_popcountll(m2 & lower) : k;
        k = w[r] >= HANDOUT_T1 ? n0 + __builtin_popcountll(m1 & lower) : k;
        k = w[r] >= HANDOUT_T0 ? __builtin_popcountll(m0 & lower) : k;
        rank[r] = (wanted >> r) & 1ull ? k : -1;
    }
    return __builtin_popcountll(wanted);
}

}  // namespace csf
