// decode_batch_plan_check.cpp -- the host-only planning of the batch decode routes (cniic_amd/csrc/decode_batch_plan.hpp) as a program of
// its own: take_chunk, the staged images' layout and the span of a route on fixed cases, then frame_dims and vor_parse_head over the
// streams tests/test_decode_batch_plan_cpu.py wrote into the directory given as argv[1] (manifest.txt: one file name per line).  Per stream one
// line: the header, the verdict, K, how many centroids the sink saw, an FNV-1a digest of what it saw, and where the parse stopped.
// Compiled with the host compiler against decode_batch_plan.hpp and huff_host.cpp, plain and under -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "decode_batch_plan.hpp"

using namespace cniic;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static std::vector<size_t> chunks(const std::vector<uint64_t> &costs, uint64_t budget) {
    std::vector<size_t> sizes;
    for (size_t i0 = 0; i0 < costs.size();) {
        const size_t i1 = take_chunk(i0, costs.size(), budget, [&](size_t i) { return costs[i]; });
        CHECK(i1 > i0);
        if (i1 <= i0) break;
        sizes.push_back(i1 - i0);
        i0 = i1;
    }
    return sizes;
}

static void check_take_chunk() {
    const std::vector<uint64_t> fives = {5, 5, 5};
    CHECK((chunks(fives, 4) == std::vector<size_t>{1, 1, 1}));   // the first item always fits
    CHECK((chunks(fives, 10) == std::vector<size_t>{2, 1}));
    CHECK((chunks(fives, 15) == std::vector<size_t>{3}));
    CHECK((chunks(fives, 14) == std::vector<size_t>{2, 1}));
    CHECK(take_chunk(0, 0, 100, [](size_t) -> uint64_t { return 1; }) == 0);
    CHECK(take_chunk(7, 7, 100, [](size_t) -> uint64_t { return 1; }) == 7);   // n = i0: nothing to take
    CHECK((chunks({0, 0, 0, 0}, 0) == std::vector<size_t>{4}));                 // a cost of 0 never ends a chunk
    CHECK((chunks({5, 0, 0, 5, 0}, 5) == std::vector<size_t>{3, 2}));
    CHECK((chunks({9, 0, 1}, 4) == std::vector<size_t>{1, 2}));                 // an item above the budget is a chunk of its own
    CHECK(take_chunk(1, 3, 10, [&](size_t i) { return fives[i]; }) == 3);
    CHECK(take_chunk(0, 2, 100, [&](size_t i) { return fives[i]; }) == 2);      // n ends it, not the budget
}

static void check_layout() {
    const uint64_t sizes[5] = {1, 15, 16, 17, 3 * 16384}, want[5] = {0, 16, 32, 48, 80};
    SlotLayout all(5);
    for (size_t i = 0; i < 5; i++) all.plan(i, sizes[i], true);
    for (size_t i = 0; i < 5; i++) CHECK(all.has(i) && all.at[i] == want[i]);
    CHECK(all.total == 80 + 3 * 16384);
    CHECK(SlotLayout::room(0) == 0 && SlotLayout::room(1) == 16 && SlotLayout::room(16) == 16 && SlotLayout::room(17) == 32);
    SlotLayout some(5);   // frames that need no slot take no room
    for (size_t i = 0; i < 5; i++) some.plan(i, sizes[i], i == 1 || i == 3);
    CHECK(!some.has(0) && !some.has(2) && !some.has(4) && some.has(1) && some.has(3));
    CHECK(some.at[1] == 0 && some.at[3] == 16 && some.total == 48);
    SlotLayout none(5);
    for (size_t i = 0; i < 5; i++) none.plan(i, sizes[i], false);
    for (size_t i = 0; i < 5; i++) CHECK(!none.has(i));
    CHECK(none.total == 0);
    SlotLayout empty(0);
    CHECK(empty.total == 0 && empty.at.empty());
}

static void check_span() {
    const uint64_t lens[6] = {7, 7, 6, 7, 7, 3};
    const ByteSpan two = frames_span(2, 5, 7, lens);   // the route {2, 5}
    CHECK(two.lo == 14 && two.hi == 38);
    const ByteSpan one = frames_span(2, 2, 7, lens);
    CHECK(one.lo == 14 && one.hi == 20);
    const ByteSpan first = frames_span(0, 0, 7, lens);
    CHECK(first.lo == 0 && first.hi == 7);
    const uint64_t big[2] = {1, 5};
    const ByteSpan far = frames_span(1, 1, 1ull << 40, big);   // 64-bit offsets
    CHECK(far.lo == (1ull << 40) && far.hi == (1ull << 40) + 5);
    CHECK(dims_fit(1, 1, 3) && !dims_fit(0, 10, 100) && !dims_fit(2, 1, 100) && !dims_fit(2, 2, 5) && dims_fit(2, 2, 6));
    CHECK(!dims_fit(0xfffffffe00000001ull, 0xffffffffull, ~0ull));   // (2^32 - 1)^2 pixels: refused before its bytes are worked out
}

static const char *name_of(VorHead v) {
    switch (v) {
    case VorHead::Ok: return "Ok";
    case VorHead::Truncated: return "Truncated";
    case VorHead::TruncatedList: return "TruncatedList";
    case VorHead::BadCentroid: return "BadCentroid";
    }
    return "?";
}

static void fnv(uint64_t &d, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; i++) { d ^= (v >> (8 * i)) & 255u; d *= 0x100000001b3ull; }
}

int main(int argc, char **argv) {
    check_take_chunk();
    check_layout();
    check_span();
    printf("plan: %d failures\n", failures);
    if (argc < 2) return failures ? 1 : 0;
    const std::string dir = argv[1];
    std::ifstream manifest(dir + "/manifest.txt");
    std::string name;
    size_t files = 0;
    while (std::getline(manifest, name)) {
        if (name.empty()) continue;
        std::ifstream in(dir + "/" + name, std::ios::binary);
        if (!in) { printf("FAIL cannot read %s\n", name.c_str()); return 1; }
        const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        // (a copy of exactly the stream's length on the heap: a read past its end is the sanitizer's to find)
        std::vector<uint8_t> copy(text.begin(), text.end());
        const uint8_t *p = copy.data();
        const uint64_t n = copy.size();
        uint32_t w = 0, h = 0;
        uint64_t pos = 99;
        files++;
        if (!frame_dims(p, n, &w, &h, &pos)) { printf("file %s dims=0\n", name.c_str()); continue; }
        CHECK(pos == 8);
        uint64_t K = 0, seen = 0, digest = 0xcbf29ce484222325ull;
        const VorHead v = vor_parse_head(p, n, pos, &K, [&](uint64_t k, uint32_t x, uint32_t y, uint8_t r, uint8_t g, uint8_t b) {
            CHECK(k == seen);
            seen++;
            fnv(digest, k, 8); fnv(digest, x, 4); fnv(digest, y, 4); fnv(digest, r, 1); fnv(digest, g, 1); fnv(digest, b, 1);
        });
        CHECK(v != VorHead::Ok || (seen == K && pos == 16 + 19 * K));
        CHECK(pos <= n);
        printf("file %s dims=1 w=%u h=%u verdict=%s K=%" PRIu64 " seen=%" PRIu64 " digest=%016" PRIx64 " pos=%" PRIu64 "\n", name.c_str(), w, h, name_of(v),
               v == VorHead::Truncated ? 0 : K, seen, digest, pos);
    }
    printf("%zu streams, %d failures\n", files, failures);
    return failures ? 1 : 0;
}
