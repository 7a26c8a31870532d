// Stand-alone driver of grand_plus_amd/csrc/optim_rows_layout.hpp for tests/test_host_optim_rows.py.  Reads one query per line
// on stdin:
//   list V key_0 key_1 ... key_{n-1}          (n may be 0; the keys ascend)
// and prints four lines: the head positions (is_head over i = 0 .. n - 1), lower_bound(row) for row = -1 .. V + 1, touched(row)
// (0 / 1) for row = 0 .. V - 1, and windows(n).  The keys lie in a heap block of exactly n elements, so a head test or a
// search that leaves the list is an address-sanitizer report.  Built with the address and undefined-behaviour sanitizers;
// no HIP, no GPU.
#include "optim_rows_layout.hpp"

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
        long long V = 0;
        if (!(in >> what >> V) || what != "list" || V < 1) return bad(line);
        std::vector<long long> given;
        for (long long k; in >> k;) given.push_back(k);
        const long long n = (long long)given.size();
        long long* keys = new long long[n];
        for (long long i = 0; i < n; ++i) {
            if (i > 0 && given[i] < given[i - 1]) return bad(line);
            keys[i] = given[i];
        }
        for (long long i = 0; i < n; ++i)
            if (gp_optim_rows::is_head(keys, i, V)) std::printf("%lld ", i);
        std::printf("\n");
        for (long long row = -1; row <= V + 1; ++row) std::printf("%lld ", gp_optim_rows::lower_bound(keys, n, row));
        std::printf("\n");
        for (long long row = 0; row < V; ++row) std::printf("%d ", gp_optim_rows::touched(keys, n, row) ? 1 : 0);
        std::printf("\n%lld\n", gp_optim_rows::windows(n));
        delete[] keys;
    }
    return 0;
}
