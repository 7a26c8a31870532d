// Stand-alone driver of grand_plus_amd/csrc/optim_defer_layout.hpp for tests/test_host_optim_defer.py.  Reads one query per
// line on stdin:
//   plan TICK LAST THROUGH CAPACITY      prints plan() as 0 (nothing), 1 (replay) or 2 (unserved)
//   cap C                                prints valid_capacity(C) as 0 / 1
//   new V CAPACITY TICK                  a table of V rows, all current through TICK, and an empty ring
//   catch T r r ...                      the pre-forward catch-up of the rows at tick T (through T - 1; nothing at T = 0)
//   step T r r ...                       the ring entry of step T is written; every row is brought through T - 1, then last = T
//   flush T                              every row through T
//   tamper SLOT TAG                      overwrites the tag of one ring slot
//   dump                                 prints last[0 .. V) on one line and the flag word on the next
// A row is handled the way catch_up_row of optim_defer.hip handles it: plan(), then tags_ok() for a replay, and an unserved
// row sets kFlagBit and keeps its last.  `last` and the ring lie in heap blocks of exactly V and CAPACITY elements, so a slot
// or a row outside them is an address-sanitizer report.  Built with the address and undefined-behaviour sanitizers; no HIP,
// no GPU.
#include "optim_defer_layout.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace gp_optim_defer;

static int bad(const std::string& line)
{
    std::fprintf(stderr, "bad query: %s\n", line.c_str());
    return 2;
}

struct Table {
    long long V = 0;
    int capacity = 0;
    int* last = nullptr;
    Entry* hist = nullptr;
    int flag = 0;
};

static bool catch_up_row(Table& t, long long row, unsigned long long tick, long long through)
{
    const long long last = t.last[row];
    const Plan what = plan(tick, last, through, t.capacity);
    if (what == kNothing) return true;
    if (what == kUnserved || !tags_ok(t.hist, last, through, t.capacity)) {
        t.flag |= kFlagBit;
        return false;
    }
    t.last[row] = (int)through;
    return true;
}

int main()
{
    Table t;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "plan") {
            unsigned long long tick;
            long long last, through;
            int capacity;
            if (!(in >> tick >> last >> through >> capacity)) return bad(line);
            std::printf("%d\n", (int)plan(tick, last, through, capacity));
        } else if (what == "cap") {
            long long c;
            if (!(in >> c)) return bad(line);
            std::printf("%d\n", valid_capacity(c) ? 1 : 0);
        } else if (what == "new") {
            long long tick;
            delete[] t.last;
            delete[] t.hist;
            if (!(in >> t.V >> t.capacity >> tick) || t.V < 1 || !valid_capacity(t.capacity)) return bad(line);
            t.last = new int[t.V];
            t.hist = new Entry[t.capacity]();
            t.flag = 0;
            for (long long r = 0; r < t.V; ++r) t.last[r] = (int)tick;
        } else if (what == "catch" || what == "step") {
            long long T;
            if (!t.last || !(in >> T) || T < 0) return bad(line);
            if (what == "step") {
                Entry e = {0.0f, 0.0f, 1.0f, tag(T)};
                t.hist[slot(T, t.capacity)] = e;
            }
            for (long long r; in >> r;) {
                if (r < 0 || r >= t.V) return bad(line);
                if (what == "catch") {
                    if (T > 0) catch_up_row(t, r, (unsigned long long)T, T - 1);
                } else if (catch_up_row(t, r, (unsigned long long)T, T - 1)) {
                    t.last[r] = (int)T;
                }
            }
        } else if (what == "flush") {
            long long T;
            if (!t.last || !(in >> T) || T < 0) return bad(line);
            for (long long r = 0; r < t.V; ++r) catch_up_row(t, r, (unsigned long long)T, T);
        } else if (what == "tamper") {
            long long s, g;
            if (!t.hist || !(in >> s >> g) || s < 0 || s >= t.capacity) return bad(line);
            t.hist[s].tag = (uint32_t)g;
        } else if (what == "dump") {
            if (!t.last) return bad(line);
            for (long long r = 0; r < t.V; ++r) std::printf("%d ", t.last[r]);
            std::printf("\n%d\n", t.flag);
        } else {
            return bad(line);
        }
    }
    delete[] t.last;
    delete[] t.hist;
    return 0;
}
