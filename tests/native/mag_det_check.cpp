// Stand-alone driver of grand_plus_amd/csrc/mag_det_layout.hpp for tests/test_host_mag_det.py.  Reads one query per line on stdin:
//   layout max_entries len_0 len_1 ... len_{n-1}
// and prints on one line: total, live_entries, tail_begin, overflowed (0 / 1), slot_of(-1), slot_of(total),
// slot_of(total + 1), then slot_of(j) for j = 0 .. total - 1.  slot_base is the exclusive prefix sum of the lengths in a
// heap block of exactly n + 1 elements, so a search that leaves it is an address-sanitizer report.  Built with the address and
// undefined-behaviour sanitizers; no HIP, no GPU.
#include "mag_det_layout.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static int bad(const std::string& line)
{
    std::fprintf(stderr, "bad query: %s\n", line.c_str());
    return 2;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string what;
        long long max_entries = 0;
        if (!(in >> what >> max_entries) || what != "layout" || max_entries < 1) return bad(line);
        std::vector<long long> len;
        for (long long v; in >> v;) {
            if (v < 0) return bad(line);
            len.push_back(v);
        }
        if (len.empty()) return bad(line);
        const long long n = (long long)len.size();
        long long* base = new long long[n + 1];
        base[0] = 0;
        for (long long e = 0; e < n; ++e) base[e + 1] = base[e] + len[e];
        const long long total = base[n];
        std::printf("%lld %lld %lld %d %lld %lld %lld", total, gp_mag_det::live_entries(total, max_entries),
                    gp_mag_det::tail_begin(total, max_entries), gp_mag_det::overflowed(total, max_entries) ? 1 : 0,
                    gp_mag_det::slot_of(base, n, -1), gp_mag_det::slot_of(base, n, total), gp_mag_det::slot_of(base, n, total + 1));
        for (long long j = 0; j < total; ++j) std::printf(" %lld", gp_mag_det::slot_of(base, n, j));
        std::printf("\n");
        delete[] base;
    }
    return 0;
}
