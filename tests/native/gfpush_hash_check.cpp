// Stand-alone driver of grand_plus_amd/csrc/gfpush_hash.hpp for tests/test_host_collision_cases.py: reads one `key cap parts`
// line per query on stdin and prints
//   hash_a hash_b home_lds(key, cap) sk_home(key, cap) sk_cell(key) slot_of(hash_b(key), parts) slot_of(hash_a(key), cap)
// A first line `consts` prints kMaxProbe and kProbeSpan.  Built with the address and undefined-behaviour sanitizers; no HIP, no GPU.
#include "gfpush_hash.hpp"

#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        if (line == "consts") { std::printf("%u %u\n", gp::kMaxProbe, gp::kProbeSpan); continue; }
        std::istringstream in(line);
        uint64_t key = 0, cap = 0, parts = 0;
        if (!(in >> key >> cap >> parts) || key > 0xFFFFFFFFull || cap <= gp::kProbeSpan || cap > 0xFFFFFFFFull || parts == 0 || parts > 0xFFFFFFFFull) {
            std::fprintf(stderr, "bad query: %s\n", line.c_str());
            return 2;
        }
        const uint32_t k = (uint32_t)key, c = (uint32_t)cap, p = (uint32_t)parts;
        std::printf("%u %u %u %u %u %u %u\n", gp::hash_a(k), gp::hash_b(k), gp::home_lds(k, c), gp::sk_home(k, c), gp::sk_cell(k),
                    gp::slot_of(gp::hash_b(k), p), gp::slot_of(gp::hash_a(k), c));
    }
    return 0;
}
