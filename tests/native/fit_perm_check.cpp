// Stand-alone driver of grand_plus_amd/csrc/fit_perm.hpp for tests/test_host_fit.py.  Reads one query per line on stdin:
//   perm key n i        prints perm(key, n, i)
//   all key n           prints perm(key, n, 0) ... perm(key, n, n - 1) on one line
//   slice t n_train bs  prints epoch lo n_labeled of step t
//   keys base epoch seed   prints epoch_key(base, epoch) and unlabel_key(seed)
//   consts              prints the three multipliers and the number of rounds
// The header takes its mixer as an argument (on the device that is gp_common.hpp's mix64); the one here is the host's
// splitmix64 step, the same formula as grand_plus_amd._common._mix.  Built with the address and undefined-behaviour
// sanitizers; no HIP, no GPU.
#include "fit_perm.hpp"

#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

static uint64_t host_mix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

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
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", (uint64_t)GP_FIT_ROUND_MUL, (uint64_t)GP_FIT_EPOCH_MUL,
                        (uint64_t)GP_FIT_UNLABEL_MUL, gp_fit::kRounds);
        } else if (what == "perm") {
            uint64_t key = 0, n = 0, i = 0;
            if (!(in >> key >> n >> i) || n < 1 || n >= (1ull << 31) || i >= n) return bad(line);
            std::printf("%u\n", gp_fit::perm(host_mix, key, (uint32_t)n, (uint32_t)i));
        } else if (what == "all") {
            uint64_t key = 0, n = 0;
            if (!(in >> key >> n) || n < 1 || n >= (1ull << 31)) return bad(line);
            for (uint64_t i = 0; i < n; ++i) std::printf(i ? " %u" : "%u", gp_fit::perm(host_mix, key, (uint32_t)n, (uint32_t)i));
            std::printf("\n");
        } else if (what == "slice") {
            uint64_t t = 0, n_train = 0, bs = 0;
            if (!(in >> t >> n_train >> bs) || t < 1 || n_train < 1 || n_train >= (1ull << 31) || bs < 1 || bs >= (1ull << 31)) return bad(line);
            const gp_fit::StepSlice s = gp_fit::step_slice(t, (uint32_t)n_train, (uint32_t)bs);
            std::printf("%" PRIu64 " %u %u\n", s.epoch, s.lo, s.n_labeled);
        } else if (what == "keys") {
            uint64_t base = 0, epoch = 0, seed = 0;
            if (!(in >> base >> epoch >> seed)) return bad(line);
            std::printf("%" PRIu64 " %" PRIu64 "\n", gp_fit::epoch_key(host_mix, base, epoch), gp_fit::unlabel_key(host_mix, seed));
        } else {
            return bad(line);
        }
    }
    return 0;
}
