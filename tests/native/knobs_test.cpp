// csrc/lnb_knobs.h on the host: the one parse rule, the two lifetimes, and the table's names.  g++ -std=c++17, no HIP.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_knobs.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static const char* name_of(Knob k) { return LNB_KNOB_TABLE[(int)k].name; }
static void set(Knob k, const char* v) { if (v) setenv(name_of(k), v, 1); else unsetenv(name_of(k)); }

int main() {
    // ---- the table: LNB_ names, unique, one row per enumerator
    CHECK(sizeof LNB_KNOB_TABLE / sizeof LNB_KNOB_TABLE[0] == (size_t)Knob::COUNT);
    std::set<std::string> seen;
    for (const KnobInfo& i : LNB_KNOB_TABLE) {
        CHECK(strncmp(i.name, "LNB_", 4) == 0 && strlen(i.name) > 4);
        CHECK(seen.insert(i.name).second);
        CHECK(i.life == ONCE || i.life == LIVE);
    }
    // ---- the parse rule on a LIVE knob (default -1): unset and empty = the default, anything else through atoi
    const Knob live = Knob::GS_TT;
    CHECK(LNB_KNOB_TABLE[(int)live].life == LIVE && LNB_KNOB_TABLE[(int)live].dflt == -1);
    set(live, nullptr); CHECK(knob(live) == -1);
    set(live, "");      CHECK(knob(live) == -1);
    set(live, "0");     CHECK(knob(live) == 0);
    set(live, "1");     CHECK(knob(live) == 1);
    set(live, "-3");    CHECK(knob(live) == -3);
    set(live, "7x y");  CHECK(knob(live) == 7);
    set(live, "zz");    CHECK(knob(live) == 0);
    set(live, nullptr); CHECK(knob(live) == -1);             // ... and it follows every change
    // ---- the same rule on ONCE knobs (one first read each: a process reads a ONCE knob once)
    const struct { Knob k; const char* v; int want; } once[] = {
        {Knob::GS_ORDER, nullptr, -1}, {Knob::NORM_ROWS_WIDE, "", 1}, {Knob::GS_NTW_CHAIN, "0", 0}, {Knob::GEMM_TILE, "1", 1},
        {Knob::FAST_GEMM_2WG, "-2", -2}, {Knob::FAST_GRID_CAP, "12abc", 12},
    };
    for (const auto& c : once) {
        CHECK(LNB_KNOB_TABLE[(int)c.k].life == ONCE);
        set(c.k, c.v);
        CHECK(knob(c.k) == c.want);
        set(c.k, "99");                                      // a ONCE knob keeps its first value
        CHECK(knob(c.k) == c.want);
        set(c.k, nullptr);
        CHECK(knob(c.k) == c.want);
    }
    // a cached 0 is a value, not "unread"
    set(Knob::GS_NTW_CHAIN, "4"); CHECK(knob(Knob::GS_NTW_CHAIN) == 0);
    if (!fails) printf("knobs_test: ok (%d knobs)\n", (int)Knob::COUNT);
    return fails ? 1 : 0;
}
