// persist_layout_check.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_wide_chunks.py builds it with -fsanitize=address,undefined).
//
// The persistent slab of a gap (fig_engine_sched.h: fig_persist_layout) and the packer's sizing of all of them (fig_pack.h:
// fig_pack_persist) for slot counts up to the wide cap.  For random (capGg, nU, nP, range, slots): the layout is asked for its
// size, laid out on a heap block of exactly that size, and every array and every part of every slot is written in full --
// the sanitizer sees a write past the block -- while the regions are checked to follow each other without overlap and the last
// slot to end at the returned size.  Then the packer's offsets for a batch of such gaps, the same way on one block.
#define FIG_EMU 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../include/figbird_hip.h"
#include "../../figbird_amd/csrc/fig_engine.h"
#include "../../figbird_amd/csrc/fig_pack.h"

struct Region { const unsigned char *p; long long n; const char *name; };

static int fail(const char *what, long long a, long long b) { printf("FAILED: %s (%lld, %lld)\n", what, a, b); return 1; }

// lays the gap out at `base`, writes all of it, returns 0 when the regions tile [base, base + size) in order
static int check_gap(unsigned char *base, long long size, int capGg, int nU, int nP, int range, int nslots, unsigned char tag) {
    FigPersist P;
    const long long got = fig_persist_layout(base, capGg, nU, nP, range, nslots, sizeof(FigState), &P);
    if (got != size) return fail("size differs between the sizing and the laying-out call", got, size);
    std::vector<Region> r = {
        {P.state, (long long)sizeof(FigState), "state"}, {P.best, capGg + 8, "best"}, {P.orig, capGg + 8, "orig"}, {P.prev, capGg + 8, "prev"},
        {P.saved, nU + 8, "saved"}, {(unsigned char *)P.org, 4 * (2LL * nU + 2), "org"}, {(unsigned char *)P.ppos_org, 4 * (3LL * nP + 3), "ppos_org"},
        {(unsigned char *)P.repeatflag, 4 * (3LL * nP + 3), "repeatflag"}, {(unsigned char *)P.used_read_arr, 4 * ((long long)range + 2), "used_read_arr"},
        {(unsigned char *)P.lrmd, 4 * (2LL * range + 4), "lrmd"}, {(unsigned char *)P.org_spec, 4 * (2LL * nU + 2), "org_spec"},
        {(unsigned char *)P.ppos_spec, 4 * (3LL * nP + 3), "ppos_spec"}};
    for (int s = 0; s < nslots; s++) {
        r.push_back({(unsigned char *)fig_slot_hdr(P, s), (long long)sizeof(FigSlot), "slot header"});
        r.push_back({fig_slot_cons(P, s), capGg + 8, "slot consensus"});
        r.push_back({fig_slot_prev(P, s, capGg), capGg + 8, "slot previous_str"});
        r.push_back({fig_slot_mark(P, s, capGg), nU + 8, "slot mark_accepted"});
    }
    const unsigned char *at = base;
    for (const Region &g : r) {
        if (g.p < at) return fail(g.name, (long long)(g.p - base), (long long)(at - base));      // overlaps its predecessor
        if (((uintptr_t)g.p & 7) != 0) return fail("region not 8-byte aligned", (long long)(g.p - base), 0);
        memset((void *)g.p, tag, (size_t)g.n);
        at = g.p + g.n;
    }
    if (at > base + size) return fail("last region ends past the size", (long long)(at - base), size);
    if (P.slots + P.slot_stride * nslots != base + size) return fail("last slot does not end at the size", (long long)(P.slots + P.slot_stride * nslots - base), size);
    if (fig_slot_mark(P, nslots - 1, capGg) + nU + 8 > base + size) return fail("last slot's mark array", 0, 0);
    return 0;
}

int main() {
    std::mt19937 rng(20260103);
    auto pick = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
    const int caps[] = {64, 128, 256, 512};
    long long cases = 0;
    for (int it = 0; it < 600; it++) {
        const int capGg = 8 * pick(1, 200), nU = pick(0, 3000), nP = pick(0, 3001), range = pick(1, 900), W = caps[pick(0, 3)];
        const int nslots = it % 3 == 0 ? std::min(range, W) : pick(1, W);
        const long long size = fig_persist_layout(nullptr, capGg, nU, nP, range, nslots, sizeof(FigState), nullptr);
        unsigned char *blk = (unsigned char *)malloc((size_t)size);
        if (check_gap(blk, size, capGg, nU, nP, range, nslots, (unsigned char)it)) { printf("  capGg=%d nU=%d nP=%d range=%d nslots=%d\n", capGg, nU, nP, range, nslots); return 1; }
        free(blk);
        cases++;
    }
    // the packer's sizing: a batch of gaps, every wide cap
    for (int it = 0; it < 40; it++) {
        FigPacked K;
        K.nslots_wide = it % 4 == 0 ? K.nslots : caps[pick(0, 3)];
        K.gaps.assign((size_t)pick(1, 60), FigDevGap());
        for (FigDevGap &d : K.gaps) { d.capGg = 8 * pick(1, 160); d.nU = pick(0, 1500); d.nP = pick(0, 800); d.rangeCap = it % 5 == 0 ? 1 : pick(1, 900); }
        fig_pack_persist(K, sizeof(FigState));
        unsigned char *blk = (unsigned char *)malloc((size_t)K.persist_total);      // (the library adds 256 bytes; none are needed)
        long long at = 0;
        for (size_t g = 0; g < K.gaps.size(); g++) {
            const FigDevGap &d = K.gaps[g];
            if (d.nslots != std::max(1, std::min(d.rangeCap, K.nslots_wide))) return fail("slots of a gap", d.nslots, d.rangeCap);
            if (d.persistOff < at || (d.persistOff & 255)) return fail("a gap's slab starts inside its predecessor or off its 256-byte line", d.persistOff, at);
            const long long size = fig_persist_layout(nullptr, d.capGg, d.nU, d.nP, d.rangeCap, d.nslots, sizeof(FigState), nullptr);
            if (check_gap(blk + d.persistOff, size, d.capGg, d.nU, d.nP, d.rangeCap, d.nslots, (unsigned char)g)) return 1;
            at = d.persistOff + size;
            cases++;
        }
        if (at > K.persist_total) return fail("the last gap's slab ends past persist_total", at, K.persist_total);
        free(blk);
    }
    printf("persist layout ok: %lld slabs\n", cases);
    return 0;
}
