// Stand-alone driver of grand_plus_amd/csrc/gather_chunk_layout.hpp for tests/test_host_gather_chunk.py.  Reads one query per line
// on stdin:
//   ok C                      prints chunk_ok(C) as 0 / 1
//   slots C n_0 n_1 ...       the segments of those lengths one after another from position 0.  Prints scratch_rows and
//                             scratch_bytes (width 7) for their total, then per segment: chunk_count, and for every chunk p
//                             its chunk_start and, for a segment of more than C positions, its slot_of (-1 otherwise)
//   where C q0 n              for every q in [q0, q0 + n): chunk_of(q, q0, C) and starts_chunk(q, q0, C) as 0 / 1
//   keys C k_0 k_1 ...        a key array as it stands, sorted or not, in a heap block of exactly that many elements, so
//                             that a read outside it is an address-sanitizer report.  Prints scratch_rows, the largest
//                             slot_of(q, p, C) over every position q and p in {0, 1, 5}, then for every window base
//                             b = 64, 128, ... below the length: seg_start_of(keys, b, keys[b]) where keys[b - 1] == keys[b]
//                             (-1 elsewhere), then is_long(keys, len, q, keys[q], C) as 0 / 1 for every q.
// Built with the address and undefined-behaviour sanitizers; no HIP, no GPU.
#include "gather_chunk_layout.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace gc = gp_gather_chunk;

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
        long long C = 0;
        if (!(in >> what >> C)) return bad(line);
        std::vector<long long> v;
        for (long long x; in >> x;) v.push_back(x);
        if (what == "ok") {
            std::printf("%d\n", gc::chunk_ok(C) ? 1 : 0);
            continue;
        }
        if (!gc::chunk_ok(C)) return bad(line);
        if (what == "slots") {
            long long total = 0;
            for (long long n : v) {
                if (n < 1) return bad(line);
                total += n;
            }
            std::printf("%lld %lld", gc::scratch_rows(total, C), gc::scratch_bytes(total, C, 7));
            long long q0 = 0;
            for (long long n : v) {
                const long long P = gc::chunk_count(n, C);
                std::printf(" %lld", P);
                for (long long p = 0; p < P; ++p) {
                    const long long q = gc::chunk_start(q0, p, C);
                    std::printf(" %lld %lld", q, n > C ? gc::slot_of(q, p, C) : -1);
                }
                q0 += n;
            }
            std::printf("\n");
        } else if (what == "where") {
            if (v.size() != 2 || v[0] < 0 || v[1] < 1) return bad(line);
            for (long long q = v[0]; q < v[0] + v[1]; ++q)
                std::printf("%s%lld %d", q == v[0] ? "" : " ", gc::chunk_of(q, v[0], C), gc::starts_chunk(q, v[0], C) ? 1 : 0);
            std::printf("\n");
        } else if (what == "keys") {
            if (v.empty()) return bad(line);
            const long long n = (long long)v.size();
            long long* keys = new long long[n];
            for (long long q = 0; q < n; ++q) keys[q] = v[q];
            long long top = -1;
            for (long long q = 0; q < n; ++q)
                for (long long p : {0ll, 1ll, 5ll}) top = gc::slot_of(q, p, C) > top ? gc::slot_of(q, p, C) : top;
            std::printf("%lld %lld", gc::scratch_rows(n, C), top);
            for (long long b = 64; b < n; b += 64)
                std::printf(" %lld", keys[b - 1] == keys[b] ? gc::seg_start_of(keys, b, keys[b]) : -1);
            for (long long q = 0; q < n; ++q) std::printf(" %d", gc::is_long(keys, n, q, keys[q], C) ? 1 : 0);
            std::printf("\n");
            delete[] keys;
        } else {
            return bad(line);
        }
    }
    return 0;
}
