// Stand-alone driver of grand_plus_amd/csrc/fit_rows_layout.hpp for tests/test_host_fit_rows.py.  Reads one query per line on
// stdin:
//   own V cap                     the ownership of the dirty bitmap's words by the waves of the snapshot's grid, walked as the
//                                 kernel walks it: every wave, every trip.  A heap block of exactly words(V) counters takes one
//                                 increment per owned word.
//     prints words(V), grid, waves, trips, the least and the greatest count of a word, how many (wave, trip) pairs fell
//     past the last word, and how many words were owned on a trip other than the first
//   copy V per_row w word         the copy of word w holding `word`, lane by lane and pass by pass: a heap block of exactly
//                                 V * per_row counters takes one increment per unit copied.
//     prints the group's log2, the passes, the greatest count of a unit, then the rows every unit of which was copied
//     exactly once; a row copied in part is printed negated minus one
//   row r                         prints word_of(r) and bit_of(r), from row_mark_layout.hpp, which this header reuses
// A word owned past the map or a unit copied past the table is an address-sanitizer report.  Built with the address and
// undefined-behaviour sanitizers; no HIP, no GPU.
#include "fit_rows_layout.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace fr = gp_fit_rows;
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
        } else if (what == "own") {
            long long V, cap;
            if (!(in >> V >> cap) || V < 1 || cap < 1) return bad(line);
            const long long n_words = rm::words(V), grid = fr::grid(n_words, cap), n_waves = grid * fr::kWaves;
            const long long n_trips = fr::trips(n_words, n_waves);
            int* owned = new int[n_words]();
            long long past = 0, later = 0;
            for (long long wave = 0; wave < n_waves; ++wave)
                for (long long trip = 0; trip < n_trips; ++trip) {
                    const long long w = fr::owned_word(wave, trip, n_waves);
                    if (w >= n_words) { ++past; break; }                              // the kernel's break
                    ++owned[w];
                    if (trip > 0) ++later;
                }
            int lo = owned[0], hi = owned[0];
            for (long long w = 1; w < n_words; ++w) {
                if (owned[w] < lo) lo = owned[w];
                if (owned[w] > hi) hi = owned[w];
            }
            std::printf("%lld %lld %lld %lld %d %d %lld %lld\n", n_words, grid, n_waves, n_trips, lo, hi, past, later);
            delete[] owned;
        } else if (what == "copy") {
            long long V, per_row, w;
            unsigned long long given;
            if (!(in >> V >> per_row >> w >> given) || V < 1 || per_row < 1 || w < 0 || w >= rm::words(V)) return bad(line);
            const unsigned bits = fr::live_bits((unsigned)given, w, V);
            const int n = rm::popcount(bits), g = fr::group_log2(per_row), n_passes = fr::passes(n, g);
            int* units = new int[V * per_row]();
            for (int pass = 0; pass < n_passes; ++pass)
                for (int lane = 0; lane < fr::kLanes; ++lane) {
                    const int k = fr::lane_slot(lane, pass, g);
                    if (k >= n) continue;
                    const long long at = fr::nth_row(bits, w, k) * per_row;
                    for (long long j = fr::lane_first(lane, g); j < per_row; j += 1 << g) ++units[at + j];
                }
            int most = 0;
            std::vector<long long> rows;
            for (long long r = 0; r < V; ++r) {
                long long once = 0, some = 0;
                for (long long j = 0; j < per_row; ++j) {
                    const int c = units[r * per_row + j];
                    if (c > most) most = c;
                    once += c == 1;
                    some += c > 0;
                }
                if (once == per_row) rows.push_back(r);
                else if (some) rows.push_back(-r - 1);
            }
            std::printf("%d %d %d", g, n_passes, most);
            for (long long r : rows) std::printf(" %lld", r);
            std::printf("\n");
            delete[] units;
        } else {
            return bad(line);
        }
    }
    return 0;
}
