// flow_i8_items.h -- how the int8 flow sweep (ssd_flow_i8.hip) splits a step's rows into wave items.  Host code without HIP: the stand-alone
// check tests/i8_items_check.cpp includes it.
//
// A wave item is a strip of 16 pixels times two consecutive output rows (the last pair of an odd Ho is shifted upwards and stores its own
// row only) or times one row.  Items are numbered strip by strip, rows downwards.  All items of one kind take the same time, and the
// device holds `slots` waves at once, so a grid runs in rounds of `slots` items and a round that is nearly empty costs a whole one:
// 1080p is 61478 two-row items, 20.01 rounds of 3072.  The plan keeps the whole rounds of two-row items (n2 of them) and gives the rows behind
// them, in the same order, to one-row items where the model says that the step ends sooner: a one-row item runs the same 33 steps with
// 12 MFMAs per step against a two-row item's 15 (the two rows share the products of six image rows) and the same loads, kI8OneRowCost of
// a two-row item's time (0.61 measured at VGA when a two-row step still took 24 MFMAs: EXPERIMENTS.md, rounds 9 and 13).  A grid below one
// round of two-row items becomes one-row items for the same reason: twice the waves, each about half as long.
#pragma once

constexpr double kI8OneRowCost = 0.6;

struct I8ItemPlan {
    int nrp;            // two-row items per strip if every row went to one: ceil(Ho / 2)
    long long n2;       // items 0 .. n2 - 1 are two-row items: item i is strip i / nrp, rows 2 (i % nrp), + 1
    long long row0;     // item n2 + j is the one-row item of linear row row0 + j: strip (row0 + j) / Ho, row (row0 + j) % Ho
    long long n1;       // one-row items
    long long last;     // items of the final round
    long long rounds;   // rounds of `slots` items (two-row rounds, then one-row rounds)
};

inline I8ItemPlan flow_i8_item_plan(int Ho, int nstrips, long long slots) {
    I8ItemPlan p{};
    if (slots < 1) slots = 1;
    p.nrp = (Ho + 1) / 2;
    const long long total2 = (long long)nstrips * p.nrp, rows = (long long)nstrips * Ho;
    const long long full = total2 / slots * slots;                                   // the whole rounds of two-row items
    const long long r0 = full / p.nrp * Ho + 2 * (full % p.nrp), n1 = rows - r0;     // (full < total2 wherever n1 > 0: no shifted pair before it)
    const long long rounds_uniform = (total2 + slots - 1) / slots, rounds1 = (n1 + slots - 1) / slots;
    const bool mixed = Ho >= 2 && n1 > 0 && (double)(full / slots) + kI8OneRowCost * (double)rounds1 < (double)rounds_uniform;
    if (Ho < 2) {   // one-row items only
        p.n2 = 0; p.row0 = 0; p.n1 = rows; p.rounds = (rows + slots - 1) / slots;
    } else if (mixed) {
        p.n2 = full; p.row0 = r0; p.n1 = n1; p.rounds = full / slots + rounds1;
    } else {
        p.n2 = total2; p.row0 = rows; p.n1 = 0; p.rounds = rounds_uniform;
    }
    const long long tail = p.n1 ? p.n1 : p.n2;
    p.last = tail - (tail - 1) / slots * slots;
    return p;
}
