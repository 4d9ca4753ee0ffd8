/* lane_merge_check.cpp -- TEST INFRASTRUCTURE: rtl-wmbus_amd/csrc/wm_lane_merge.h (how a batch lane orders the recorded stream
 * operations of its two contexts) over random operation lists, on the host alone.  For every pair of lists:
 *   - the output holds every operation of A and of B exactly once, each list's in its own order;
 *   - a paired step joins two operations that may pair (same pairable kernel, same block and LDS size), and nothing else;
 *   - whenever both lists stood at operations that may pair, that step paired them;
 *   - lists without a pairable operation come out as A followed by B;
 *   - TURNS: runs of kind-0 operations of either list are bracketed as turns (the demodulation kernel's turn: "taking the K1 turn"
 *     ... "handing on the K1 turn", K1Turn in wm_api.hip; here a side array over the operations, WmLaneKey has no such field).  No
 *     step that carries an operation of the OTHER list falls between the first and the last operation of a turn: the recorded
 *     take() of the mate would find the chain held and return hipErrorInvalidValue.
 *     PRECONDITION, which the lists drawn here keep and the library keeps today: nothing pairable is recorded between take() and
 *     hand_on().  Without it the property is false: A = [P3, 0, 0] (a turn over its two kind-0 operations), B = [0, P2, 0] (a turn
 *     over all three, P2 inside it) comes out as B's take, A's P3, A's take -- two turns open at once.
 * Real push shapes (front_list / back_list below write out what enqueue_front_impl and enqueue_back_impl record): for every pair of
 * the variants a lane meets -- rounds or none, spans or none, a clock kernel with a paired form or without, cooperative or not, a
 * mate with no push at all -- in both orders, the merge pairs as many launches as the longest common subsequence of the two lists'
 * pairable operations holds (computed here from the lists, not from the merge); where one list's pairable operations are a
 * subsequence of the other's that is every one of the shorter list.
 * NOT asserted, because it is false: maximal pairing of arbitrary lists.  The rule looks ahead from A's head only, so how much pairs
 * depends on which list is A: A = [P1, P2, P1], B = [P2, P1] pairs once, B against A pairs twice.  Known and accepted: the lists of
 * two mates differ by launches one of them lacks, not by launches in another order.
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

/* turns over a list: some of its runs of kind-0 operations (two or more), numbered from 1; 0: the operation is in no turn */
static std::vector<uint32_t> make_turns(const std::vector<WmLaneKey> &L)
{
    std::vector<uint32_t> turn(L.size(), 0u);
    uint32_t id = 0;
    for (size_t i = 0; i < L.size();) {
        size_t e = i;
        while (e < L.size() && L[e].kind == 0u) e++;
        if (e == i) { i++; continue; }
        if (e - i >= 2u && rnd(3)) {                                             /* a turn inside the run [i, e): never over a pairable operation */
            const size_t first = i + rnd((uint32_t)(e - i - 1u)), last = first + 1u + rnd((uint32_t)(e - first - 1u));
            id++;
            for (size_t k = first; k <= last; k++) turn[k] = id;
        }
        i = e;
    }
    return turn;
}

/* no step with an operation of one list between the first and the last operation of a turn of the other */
static bool turns_kept(const std::vector<WmLaneKey> &A, const std::vector<uint32_t> &ta, const std::vector<WmLaneKey> &B, const std::vector<uint32_t> &tb)
{
    uint32_t open_a = 0, open_b = 0;                                             /* the turn either list is inside after the steps so far */
    bool ok = true;
    wm_lane_merge(A.data(), A.size(), B.data(), B.size(), [&](long a, long b) {
        if (a >= 0 && open_b) ok = false;
        if (b >= 0 && open_a) ok = false;
        if (a >= 0) open_a = ta[(size_t)a] && (size_t)a + 1u < A.size() && ta[(size_t)a + 1u] == ta[(size_t)a] ? ta[(size_t)a] : 0u;
        if (b >= 0) open_b = tb[(size_t)b] && (size_t)b + 1u < B.size() && tb[(size_t)b + 1u] == tb[(size_t)b] ? tb[(size_t)b] : 0u;
    });
    return ok && !open_a && !open_b;
}

/* ---- the lists a push records (wm_api.hip: enqueue_front_impl, enqueue_back_impl, launch_k3), as keys ---------------------------------- */
enum : uint64_t { K_CLK_COOP = 1, K_CLK_LANE, K_CLK_LIST, K_RLA, K_RLA_LIST, K_SCAN, K_SPANS, K_BURSTS };
struct Shape {
    bool present;        /* the mate has a push in this half at all (else: its source has ended, an empty list) */
    unsigned rounds;     /* unattended list rounds per framer (0: a push of one segment per row) */
    bool clock_pairs;    /* the systolic clock form (clock_waves = 1: the one-wave form has no paired launch) */
    bool coop;           /* whole waves of captures: the cooperative first pass, another kernel than the lane-by-lane one */
    bool spans;          /* RSSI on demand: k3_spans and the RSSI relaunch (off: every sample, or the paused mode) */
    bool stages;         /* line_levels, crc_repair, line_quality behind the bursts */
};
static const WmLaneKey PLAIN{0u, 0u, 0u};

static void front_list(const Shape &s, std::vector<WmLaneKey> &L, std::vector<uint32_t> &turn)
{
    L.clear(); turn.clear();
    if (!s.present) return;
    auto plain = [&](unsigned n, uint32_t t = 0u) { for (unsigned k = 0; k < n; k++) { L.push_back(PLAIN); turn.push_back(t); } };
    auto launch = [&](uint64_t kind, uint32_t block, uint32_t lds, bool pairs) { L.push_back(pairs ? WmLaneKey{kind, block, lds} : PLAIN); turn.push_back(0u); };
    plain(5);                                                 /* staged event and wait, push event, history copy, scalars fill */
    plain(7, 1u);                                             /* the turn: take, event, demodulation head, event, tail, event, hand on */
    plain(s.spans ? 0u : 4u);                                 /* every-sample RSSI: the tile hand-off rounds and their commit */
    plain(1);
    launch(s.coop ? K_CLK_COOP : K_CLK_LANE, 256u, 8192u, s.clock_pairs);
    for (unsigned r = 0; r < s.rounds; r++) { plain(1); launch(K_CLK_LIST, 256u, 8192u, s.clock_pairs); }
    plain(1);
    launch(K_RLA, 256u, 0u, true);
    for (unsigned r = 0; r < s.rounds; r++) { plain(1); launch(K_RLA_LIST, 256u, 0u, true); }
    plain(3);                                                 /* finish, event, history copy */
}

static void back_list(const Shape &s, std::vector<WmLaneKey> &L, std::vector<uint32_t> &turn)
{
    L.clear(); turn.clear();
    if (!s.present) return;
    auto plain = [&](unsigned n) { for (unsigned k = 0; k < n; k++) { L.push_back(PLAIN); turn.push_back(0u); } };
    auto launch = [&](uint64_t kind) { L.push_back(WmLaneKey{kind, 256u, 0u}); turn.push_back(0u); };
    plain(3);                                                 /* owed chips to the device, event, chip sums */
    launch(K_SCAN);
    if (s.spans) { plain(1); launch(K_SPANS); plain(3); }     /* flags fill, spans, event, RSSI relaunch, event */
    launch(K_BURSTS);
    plain(s.stages ? 4u : 0u);                                /* levels, level tail, repair, quality */
    plain(3);                                                 /* event, scalars to the host, event */
}

/* the longest common subsequence of the two lists' pairable operations: the most launches any order-keeping merge can pair */
static unsigned most_pairs(const std::vector<WmLaneKey> &A, const std::vector<WmLaneKey> &B)
{
    std::vector<WmLaneKey> a, b;
    for (const WmLaneKey &k : A) if (k.kind) a.push_back(k);
    for (const WmLaneKey &k : B) if (k.kind) b.push_back(k);
    std::vector<std::vector<unsigned>> t(a.size() + 1u, std::vector<unsigned>(b.size() + 1u, 0u));
    for (size_t i = 1; i <= a.size(); i++)
        for (size_t j = 1; j <= b.size(); j++)
            t[i][j] = wm_lane_pairs(a[i - 1u], b[j - 1u]) ? t[i - 1u][j - 1u] + 1u : (t[i - 1u][j] > t[i][j - 1u] ? t[i - 1u][j] : t[i][j - 1u]);
    return t[a.size()][b.size()];
}

static unsigned pairable_count(const std::vector<WmLaneKey> &L)
{
    unsigned n = 0;
    for (const WmLaneKey &k : L) n += k.kind != 0u;
    return n;
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
        const std::vector<uint32_t> ta = make_turns(A), tb = make_turns(B);
        cases++; wrong += !turns_kept(A, ta, B, tb);
        cases++; wrong += !turns_kept(B, tb, A, ta);
    }
    /* the precondition is needed, and turns_kept sees a broken turn: the header's counterexample, a pairable operation inside B's turn */
    {
        const std::vector<WmLaneKey> A = {{3, 256, 0}, {0, 0, 0}, {0, 0, 0}}, B = {{0, 0, 0}, {2, 256, 0}, {0, 0, 0}};
        cases++; wrong += turns_kept(A, {0u, 1u, 1u}, B, {1u, 1u, 1u});
    }
    /* the header's example of order dependence, as it stands: once one way, twice the other (a better rule changes this case and that comment together) */
    {
        const std::vector<WmLaneKey> A = {{1, 256, 0}, {2, 256, 0}, {1, 256, 0}}, B = {{2, 256, 0}, {1, 256, 0}};
        unsigned ab = 0, ba = 0;
        wm_lane_merge(A.data(), A.size(), B.data(), B.size(), [&](long a, long b) { ab += a >= 0 && b >= 0; });
        wm_lane_merge(B.data(), B.size(), A.data(), A.size(), [&](long a, long b) { ba += a >= 0 && b >= 0; });
        cases++; wrong += ab != 1u || ba != 2u;
    }
    /* the lists of real pushes, every variant against every other, fronts and backs, in both orders */
    {
        std::vector<Shape> shapes;
        shapes.push_back(Shape{false, 0u, true, true, true, false});                         /* a mate whose source has ended */
        for (unsigned rounds : {0u, 2u, 3u})
            for (int clock_pairs = 0; clock_pairs < 2; clock_pairs++)
                for (int coop = 0; coop < 2; coop++)
                    for (int spans = 0; spans < 2; spans++)
                        for (int stages = 0; stages < 2; stages++) shapes.push_back(Shape{true, rounds, clock_pairs != 0, coop != 0, spans != 0, stages != 0});
        for (const Shape &x : shapes)
            for (const Shape &y : shapes)
                for (int front = 0; front < 2; front++) {
                    std::vector<WmLaneKey> A, B;
                    std::vector<uint32_t> ta, tb;
                    if (front) { front_list(x, A, ta); front_list(y, B, tb); } else { back_list(x, A, ta); back_list(y, B, tb); }
                    unsigned pairs = 0;
                    wm_lane_merge(A.data(), A.size(), B.data(), B.size(), [&](long a, long b) { pairs += a >= 0 && b >= 0; });
                    cases++; wrong += !check(A, B, false) || !turns_kept(A, ta, B, tb) || pairs != most_pairs(A, B);
                }
        /* a mate that only LACKS launches of the full push (no rounds, no spans, no paired clock form, no push): every pairable one it has pairs */
        const Shape full{true, 2u, true, true, true, true};
        const Shape lacks[] = {{true, 0u, true, true, true, true}, {true, 2u, true, true, false, true}, {true, 2u, false, true, true, true},
                               {true, 0u, false, true, false, false}, {false, 0u, true, true, true, false}};
        for (const Shape &y : lacks)
            for (int front = 0; front < 2; front++)
                for (int swap = 0; swap < 2; swap++) {
                    std::vector<WmLaneKey> A, B;
                    std::vector<uint32_t> ta, tb;
                    if (front) { front_list(swap ? y : full, A, ta); front_list(swap ? full : y, B, tb); }
                    else { back_list(swap ? y : full, A, ta); back_list(swap ? full : y, B, tb); }
                    unsigned pairs = 0;
                    wm_lane_merge(A.data(), A.size(), B.data(), B.size(), [&](long a, long b) { pairs += a >= 0 && b >= 0; });
                    cases++; wrong += pairs != pairable_count(swap ? A : B);
                }
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
