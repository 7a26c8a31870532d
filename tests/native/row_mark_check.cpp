// Stand-alone driver of grand_plus_amd/csrc/row_mark_layout.hpp for tests/test_host_row_mark.py.  Reads one query per line on
// stdin:
//   compact V capacity word_0 ... word_{words(V)-1}     the compaction as the two launches of row_mark.hip cut it: per chunk
//                                                      the popcount of the valid bits, then emit_word at the exclusive prefix
//     prints three lines: the capacity keys; total, overflowed, tail_begin, words(V), chunks; the chunks' partial counts
//   chunks n_words                                     prints chunks, chunk_words and chunk_begin(0 .. chunks)
//   row r                                              prints word_of(r) and bit_of(r)
// The bitmap lies in a heap block of exactly words(V) words and the keys in one of exactly `capacity`, so a word read past
// the map or a key written past the capacity is an address-sanitizer report.  Built with the address and
// undefined-behaviour sanitizers; no HIP, no GPU.
#include "row_mark_layout.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace rm = gp_row_mark;

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
        if (what == "row") {
            long long r;
            if (!(in >> r) || r < 0) return bad(line);
            std::printf("%lld %u\n", rm::word_of(r), rm::bit_of(r));
        } else if (what == "chunks") {
            long long n_words;
            if (!(in >> n_words) || n_words < 0) return bad(line);
            const long long n = rm::chunks(n_words);
            std::printf("%lld %lld", n, rm::chunk_words(n_words, n));
            for (long long c = 0; c <= n; ++c) std::printf(" %lld", rm::chunk_begin(c, n_words, n));
            std::printf("\n");
        } else if (what == "compact") {
            long long V = 0, capacity = 0;
            if (!(in >> V >> capacity) || V < 1 || capacity < 1) return bad(line);
            std::vector<unsigned> given;
            for (unsigned long long x; in >> x;) given.push_back((unsigned)x);
            const long long n_words = rm::words(V);
            if ((long long)given.size() != n_words) return bad(line);
            unsigned* bitmap = new unsigned[n_words];
            for (long long w = 0; w < n_words; ++w) bitmap[w] = given[w];
            long long* keys = new long long[capacity];
            for (long long i = 0; i < capacity; ++i) keys[i] = -7;
            const long long n_chunks = rm::chunks(n_words);
            std::vector<long long> partials(n_chunks, 0);
            for (long long c = 0; c < n_chunks; ++c)                                  // the count launch
                for (long long w = rm::chunk_begin(c, n_words, n_chunks); w < rm::chunk_begin(c + 1, n_words, n_chunks); ++w)
                    partials[c] += rm::popcount(bitmap[w] & rm::valid_mask(w, V));
            long long total = 0;
            for (long long c = 0; c < n_chunks; ++c) total += partials[c];
            for (long long c = 0; c < n_chunks; ++c) {                                // the write launch
                long long prefix = 0;
                for (long long g = 0; g < c; ++g) prefix += partials[g];
                for (long long w = rm::chunk_begin(c, n_words, n_chunks); w < rm::chunk_begin(c + 1, n_words, n_chunks); ++w) {
                    prefix += rm::emit_word(bitmap[w], w, prefix, V, capacity, keys);
                    bitmap[w] = 0u;
                }
            }
            for (long long j = rm::tail_begin(total, capacity); j < capacity; ++j) keys[j] = V;
            for (long long i = 0; i < capacity; ++i) std::printf("%lld ", keys[i]);
            std::printf("\n%lld %d %lld %lld %lld\n", total, rm::overflowed(total, capacity) ? 1 : 0, rm::tail_begin(total, capacity),
                        n_words, n_chunks);
            for (long long c = 0; c < n_chunks; ++c) std::printf("%lld ", partials[c]);
            std::printf("\n");
            delete[] keys;
            delete[] bitmap;
        } else {
            return bad(line);
        }
    }
    return 0;
}
