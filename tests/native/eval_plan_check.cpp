// Stand-alone driver of grand_plus_amd/csrc/eval_plan.hpp for tests/test_host_eval_tail.py.  Reads one query per line on stdin:
//   consts     prints kSlots kMinSlice kTailSlices kTailMaxRows kTailWorkspaceBytes
//   plan n     prints grid slice of reduce_plan(n), then first and end of the first and of the last slice
// Built with the address and undefined-behaviour sanitizers; no HIP, no GPU.
#include "eval_plan.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

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
        in >> what;
        if (what == "consts") {
            std::printf("%d %d %d %lld %lld\n", gp_eval::kSlots, gp_eval::kMinSlice, gp_eval::kTailSlices, (long long)gp_eval::kTailMaxRows,
                        (long long)gp_eval::kTailWorkspaceBytes);
        } else if (what == "plan") {
            long long n = -1;
            if (!(in >> n) || n < 0) return bad(line);
            const gp_eval::ReducePlan p = gp_eval::reduce_plan(n);
            const long long last_first = (p.grid - 1) * p.slice;
            const long long first_end = p.slice < n ? p.slice : n;
            const long long last_end = last_first + p.slice < n ? last_first + p.slice : n;
            std::printf("%lld %lld 0 %lld %lld %lld\n", p.grid, p.slice, first_end, last_first, last_end);
        } else {
            return bad(line);
        }
    }
    return 0;
}
