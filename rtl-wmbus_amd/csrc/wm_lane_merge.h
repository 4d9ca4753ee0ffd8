/* wm_lane_merge.h -- the order in which a batch lane issues the recorded operations of its two contexts (wm_batch.h).
 *
 * A lane drives two receiver contexts on ONE stream.  Each context's half of a push is recorded as a list of stream
 * operations (kernel launches, fills, copies, event records, waits); this header merges two such lists into one
 * sequence.  Every context's own order is kept exactly; the contexts share no device buffers, so any such interleaving
 * computes what the two lists computed one after the other.  Where both lists stand at the SAME pairable kernel with the
 * same block and LDS size, the two launches leave as one (gridDim.z = 2, wm_k_pair.h); everything else leaves singly.
 *
 * No HIP types here: the merge is tested on the host alone (tests/lane_merge_check.cpp). */
#ifndef WM_LANE_MERGE_H
#define WM_LANE_MERGE_H

#include <stddef.h>
#include <stdint.h>

struct WmLaneKey {
    uint64_t kind;           /* which pairable kernel (0: an operation that always leaves singly) */
    uint32_t block, lds;     /* threads per block, dynamic LDS bytes */
};

static inline bool wm_lane_pairs(const WmLaneKey &x, const WmLaneKey &y)
{
    return x.kind != 0u && x.kind == y.kind && x.block == y.block && x.lds == y.lds;
}

/* emit(ia, ib): operation ia of list A alone (ib < 0), operation ib of list B alone (ia < 0), or both as one paired launch.
 * Rule: equal pairable heads pair; an operation that cannot pair leaves at once, A's first (so a run of them stays
 * together: the demodulation kernel's turn, taken and handed on by such operations, is never interleaved with the mate's);
 * two pairable heads that differ: the one whose partner waits further down the other list holds on while the other list
 * catches up.  With nothing pairable the result is A followed by B.
 *
 * PRECONDITION of "never interleaved": nothing pairable may be recorded between take() and hand_on() of a K1 turn (K1Turn,
 * wm_api.hip); today nothing is.  A pairable operation inside a turn can be held back while the mate's list runs on into a
 * turn of its own, and the second recorded take() then fails with hipErrorInvalidValue: A = [P3, 0, 0] (a turn over the two
 * plain operations), B = [0, P2, 0] (a turn over all three) leaves as B's take, A's P3, A's take -- two turns open at once.
 * How MUCH pairs depends on which list is A (the look-ahead is from A's head only): A = [P1, P2, P1], B = [P2, P1] pairs once,
 * the lists swapped pair twice.  Accepted: two mates' lists differ by launches one of them lacks, not by their order, and for
 * those every launch that can pair does (tests/lane_merge_check.cpp holds both statements). */
template <typename Emit>
static inline void wm_lane_merge(const WmLaneKey *A, size_t na, const WmLaneKey *B, size_t nb, Emit emit)
{
    size_t i = 0, j = 0;
    while (i < na && j < nb) {
        if (wm_lane_pairs(A[i], B[j])) { emit((long)i++, (long)j++); continue; }
        if (A[i].kind == 0u) { emit((long)i++, -1L); continue; }
        if (B[j].kind == 0u) { emit(-1L, (long)j++); continue; }
        bool later = false;                                 /* does A's head find its partner further down B? */
        for (size_t k = j + 1; k < nb && !later; k++) later = wm_lane_pairs(A[i], B[k]);
        if (later) emit(-1L, (long)j++); else emit((long)i++, -1L);
    }
    for (; i < na; i++) emit((long)i, -1L);
    for (; j < nb; j++) emit(-1L, (long)j);
}

#endif /* WM_LANE_MERGE_H */
