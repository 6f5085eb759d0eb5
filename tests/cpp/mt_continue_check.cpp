// TEST PROGRAM: is an exported progressive-render state the reference sampler's own?  The reference
// gives every pixel a std::mt19937_64 (IncoherentSampler, math/Sampler.h:96, seeded in main.cpp:73);
// sp_pixel_state.mt / mt_pos are documented as that engine's _M_x / _M_p.  For every record of the
// input file this builds the engine two ways and compares their next outputs:
//   a: std::mt19937_64 a(seed); a.discard(draws);          -- the reference's engine after `draws` words
//   b: the exported words streamed in with operator>>       -- what a host continuing the render loads
//
//   mt_continue_check <file>   records of {u64 seed, u64 draws, u64 mt[312], u64 mt_pos}, little endian
//   mt_continue_check --self   the same check on states this program takes from std::mt19937_64 itself
//                              (operator<<), at positions 0, 312 and in between
// Prints "<n> records, <k> mismatching" and exits 0 when k == 0.  Plain g++ -std=c++17, no GPU.
#include <cstdint>
#include <cstdio>
#include <random>
#include <sstream>
#include <string>
#include <vector>

namespace {
constexpr int N       = 312;
constexpr int OUTPUTS = 700; // more than two generations ahead

struct Record {
    uint64_t seed, draws, mt[N], mt_pos;
};

bool continues(const Record& r)
{
    std::mt19937_64 a(r.seed);
    a.discard(r.draws);
    std::ostringstream text;
    for (int k = 0; k < N; ++k) text << r.mt[k] << ' ';
    text << r.mt_pos;
    std::istringstream in(text.str());
    std::mt19937_64    b;
    in >> b;
    if (in.fail()) return false;
    for (int k = 0; k < OUTPUTS; ++k)
        if (a() != b()) return false;
    return true;
}

// a state as libstdc++ prints it: 312 words, then the position
Record state_of(uint64_t seed, uint64_t draws)
{
    std::mt19937_64 e(seed);
    e.discard(draws);
    std::ostringstream out;
    out << e;
    std::istringstream in(out.str());
    Record             r{};
    r.seed  = seed;
    r.draws = draws;
    for (int k = 0; k < N; ++k) in >> r.mt[k];
    in >> r.mt_pos;
    return r;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <file> | --self\n", argv[0]);
        return 2;
    }
    std::vector<Record> recs;
    if (std::string(argv[1]) == "--self") {
        for (uint64_t seed : { 0xb0ae9d99ull, 0x12340056ull ^ 0xb0ae9d99ull, 1ull })
            for (uint64_t draws : { 0ull, 1ull, 311ull, 312ull, 313ull, 623ull, 624ull, 10000ull })
                recs.push_back(state_of(seed, draws));
        // the position a seeded engine starts at (312) and the one after a twist (0) are both there
        bool p0 = false, p312 = false;
        for (const Record& r : recs) {
            p0   = p0 || r.mt_pos == 0;
            p312 = p312 || r.mt_pos == 312;
        }
        if (!p312) {
            std::printf("self-check: no state at position 312\n");
            return 1;
        }
        (void)p0;
        // and a corrupted state must be seen
        Record bad = recs[3];
        bad.mt[5] ^= 1;
        if (continues(bad)) {
            std::printf("self-check: a corrupted state passed\n");
            return 1;
        }
    } else {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        Record r;
        while (std::fread(&r, sizeof(r), 1, f) == 1) recs.push_back(r);
        std::fclose(f);
    }
    size_t bad = 0;
    for (const Record& r : recs) bad += continues(r) ? 0 : 1;
    std::printf("%zu records, %zu mismatching\n", recs.size(), bad);
    return bad == 0 && !recs.empty() ? 0 : 1;
}
