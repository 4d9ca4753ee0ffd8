/* lane_merge_check.cpp -- TEST INFRASTRUCTURE: rtl-wmbus_amd/csrc/wm_lane_merge.h (how a batch lane orders the recorded stream
 * operations of its two contexts) over random operation lists, on the host alone.  For every pair of lists:
 *   - the output holds every operation of A and of B exactly once, each list's in its own order;
 *   - a paired step joins two operations that may pair (same pairable kernel, same block and LDS size), and nothing else;
 *   - whenever both lists stood at operations that may pair, that step paired them;
 *   - lists without a pairable operation come out as A followed by B.
 * Prints "<cases> cases, <wrong> wrong"; exit code 1 if any was wrong.  Build: g++ -O2 -I rtl-wmbus_amd/csrc. */
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wm_lane_merge.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 20) % n);
}

struct Step { long a, b; };

/* a list the way a context records one: mostly the same sequence as its mate's, with kinds, sizes and extra operations that differ */
static std::vector<WmLaneKey> make_list(const std::vector<WmLaneKey> &base, uint32_t noise, bool pairable)
{
    std::vector<WmLaneKey> out;
    for (const WmLaneKey &k : base) {
        const uint32_t r = rnd(100);
        if (r < noise) continue;                                              /* an operation the mate has and this one lacks */
        WmLaneKey x = k;
        if (r < 2 * noise) x.kind = pairable ? 1u + rnd(4) : 0u;              /* another kernel in the same place */
        else if (r < 3 * noise) x.block = 64u << rnd(3);                      /* the same kernel with another block size */
        else if (r < 4 * noise) x.lds ^= 1024u;
        out.push_back(x);
        if (rnd(100) < noise) out.push_back(WmLaneKey{pairable && rnd(2) ? 1u + rnd(4) : 0u, 256u, 0u});
    }
    return out;
}

static bool check(const std::vector<WmLaneKey> &A, const std::vector<WmLaneKey> &B, bool none_pairable)
{
    std::vector<Step> steps;
    /* the heads as the merge saw them at every step, reconstructed from the steps taken so far */
    wm_lane_merge(A.data(), A.size(), B.data(), B.size(), [&](long a, long b) { steps.push_back(Step{a, b}); });
    size_t i = 0, j = 0;
    for (const Step &s : steps) {
        const bool heads_pair = i < A.size() && j < B.size() && wm_lane_pairs(A[i], B[j]);
        if (s.a < 0 && s.b < 0) return false;
        if (s.a >= 0 && s.b >= 0) {
            if ((size_t)s.a != i || (size_t)s.b != j || !heads_pair) return false;          /* pairs exactly the equal pairable heads ... */
            i++; j++;
        } else {
            if (heads_pair) return false;                                                  /* ... and never passes them by */
            if (s.a >= 0) { if ((size_t)s.a != i) return false; i++; }                     /* each list in its own order, nothing skipped or repeated */
            else { if ((size_t)s.b != j) return false; j++; }
        }
    }
    if (i != A.size() || j != B.size()) return false;                                      /* a permutation of both inputs */
    if (none_pairable) {                                                                    /* plain concatenation */
        if (steps.size() != A.size() + B.size()) return false;
        for (size_t k = 0; k < steps.size(); k++)
            if (k < A.size() ? steps[k].a != (long)k || steps[k].b >= 0 : steps[k].b != (long)(k - A.size()) || steps[k].a >= 0) return false;
    }
    return true;
}

int main()
{
    unsigned long cases = 0, wrong = 0;
    for (uint32_t round = 0; round < 20000; round++) {
        const bool pairable = round % 4u != 3u;                    /* every fourth round: nothing pairable at all */
        std::vector<WmLaneKey> base;
        const uint32_t n = rnd(40);
        for (uint32_t k = 0; k < n; k++) base.push_back(WmLaneKey{pairable && rnd(3) ? 1u + rnd(4) : 0u, rnd(2) ? 256u : 64u, rnd(4) ? 0u : 4096u});
        const uint32_t noise = rnd(12);
        const std::vector<WmLaneKey> A = make_list(base, noise, pairable), B = rnd(10) ? make_list(base, noise, pairable) : std::vector<WmLaneKey>();
        cases++; wrong += !check(A, B, !pairable);
        cases++; wrong += !check(B, A, !pairable);
    }
    /* identical lists of pairable operations pair throughout */
    {
        std::vector<WmLaneKey> A;
        for (uint32_t k = 0; k < 16; k++) A.push_back(WmLaneKey{1u + k % 3u, 256u, 0u});
        unsigned pairs = 0, singles = 0;
        wm_lane_merge(A.data(), A.size(), A.data(), A.size(), [&](long a, long b) { if (a >= 0 && b >= 0) pairs++; else singles++; });
        cases++; wrong += pairs != 16 || singles != 0;
    }
    /* a mate that lacks one launch: the other list holds on, everything behind it still pairs */
    {
        const std::vector<WmLaneKey> A = {{1, 256, 0}, {0, 0, 0}, {2, 256, 0}, {3, 256, 0}}, B = {{1, 256, 0}, {0, 0, 0}, {3, 256, 0}};
        unsigned pairs = 0;
        wm_lane_merge(A.data(), A.size(), B.data(), B.size(), [&](long a, long b) { pairs += a >= 0 && b >= 0; });
        cases++; wrong += pairs != 2;
        pairs = 0;
        wm_lane_merge(B.data(), B.size(), A.data(), A.size(), [&](long a, long b) { pairs += a >= 0 && b >= 0; });
        cases++; wrong += pairs != 2;
    }
    std::printf("%lu cases, %lu wrong\n", cases, wrong);
    return wrong != 0;
}
