// trie_shapes_check.cpp -- the host's three readers of a serialised decoder (cniic_amd/csrc/huff_host.cpp: huff_parse_leaves, huff_parse_trie,
// huff_decode_host) over the hand-built streams of tests/trie_shapes.py, as a stand-alone program: tests/test_trie_shapes_cpu.py compiles it
// with huff_host.cpp, plain and under -fsanitize=address,undefined, and runs it on a directory it wrote.
//
//   trie_shapes_check DIR      DIR/manifest.txt: one line per stream
//       FILE KIND SYMBOLS LEAVES DEEPEST PAYLOAD VERDICT KEYS
//   FILE the stream; KIND 1 = RGB leaves, 2 = signed ones (CNIIC_SYM_*); SYMBOLS = w h; VERDICT 1 = the reference decodes it, 0 = it refuses;
//   for a stream made whole by hand LEAVES, DEEPEST (the deepest leaf), PAYLOAD (the offset behind the trie) and KEYS, a file of SYMBOLS u32: the
//   key of every symbol, from the payload's leaf sequence; "-" and zeros for an edited or cut stream, of which only the verdict is known.
//
// Per stream: both parsers agree with the verdict and with each other (leaves in pre-order: key, depth, path); too_deep exactly when a branch
// lies at depth >= kLeafMaxLen, that is when the deepest leaf is deeper than kLeafMaxLen; leaf count, deepest leaf, payload offset; the node
// walk's keys equal the payload's leaf sequence.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "huff_host.hpp"

using namespace cniic;

static int g_fail = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            printf("FAIL %s: %s -- ", file.c_str(), #cond);                      \
            printf(__VA_ARGS__);                                                 \
            printf("\n");                                                        \
            g_fail++;                                                            \
            return;                                                              \
        }                                                                        \
    } while (0)

static bool read_file(const std::string &path, std::vector<uint8_t> &out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

struct Counts { int good = 0, refused = 0, deep = 0; uint32_t deepest = 0; uint64_t most_leaves = 0; };

static void check(const std::string &dir, const std::string &file, int kind, uint64_t nsyms, uint64_t leaves, uint32_t deepest, uint64_t payload,
                  int verdict, const std::string &keys_file, Counts &cnt) {
    std::vector<uint8_t> raw;
    CHECK(read_file(dir + "/" + file, raw), "cannot read");
    // an allocation of exactly the stream's length: a read behind it is the sanitizer's to see
    std::vector<uint8_t> s(raw.begin(), raw.end());
    s.shrink_to_fit();
    const uint64_t n = s.size();
    CHECK(n >= 8, "no dimensions");
    LeafTable lt;
    std::vector<TrieNode> nodes;
    uint64_t pl = 8, pt = 8;
    const bool ok_l = huff_parse_leaves(kind, s.data(), n, pl, lt);
    const bool ok_t = huff_parse_trie(kind, s.data(), n, pt, nodes);
    // (a table that is too deep ends the leaves' parse at once, with no verdict: the caller parses nodes instead)
    CHECK(ok_l == ok_t || (ok_l && lt.too_deep), "huff_parse_leaves %d, huff_parse_trie %d", (int)ok_l, (int)ok_t);
    bool decoded = false;
    std::vector<uint32_t> got(nsyms);
    if (ok_t) decoded = huff_decode_host(nodes, s.data() + pt, n - pt, nsyms, got.data(), nullptr);
    CHECK((ok_t && decoded) == (verdict != 0), "parsed %d, decoded %d, the reference's verdict %d", (int)ok_t, (int)decoded, verdict);
    if (!verdict) { cnt.refused++; return; }
    // the leaves of the node walk in pre-order (the nodes ARE in pre-order), with depth and path
    std::vector<uint32_t> depth(nodes.size(), 0);
    std::vector<uint64_t> path(nodes.size(), 0);
    uint64_t nl = 0;
    uint32_t deepest_t = 0;
    for (size_t i = 0; i < nodes.size(); i++) {
        if (nodes[i].l == kTrieLeaf) {
            if (!lt.too_deep) {
                CHECK(nl < lt.n(), "more leaves in the trie than in the table");
                CHECK(lt.key[nl] == nodes[i].r && lt.len[nl] == depth[i] && lt.code[nl] == path[i], "leaf %" PRIu64 ": table (%u, %u, %016" PRIx64 "), trie (%u, %u, %016" PRIx64 ")",
                      nl, lt.key[nl], (unsigned)lt.len[nl], lt.code[nl], nodes[i].r, depth[i], path[i]);
            }
            deepest_t = depth[i] > deepest_t ? depth[i] : deepest_t;
            nl++;
        } else {
            CHECK(nodes[i].l == i + 1 && nodes[i].r > i + 1 && nodes[i].r < nodes.size(), "children of node %zu", i);
            const uint32_t d = depth[i] + 1;
            depth[nodes[i].l] = depth[nodes[i].r] = d;
            path[nodes[i].l] = path[i];
            path[nodes[i].r] = d <= 64 ? path[i] | (1ull << (64 - d)) : path[i];
        }
    }
    CHECK(nodes.size() == 2 * nl - 1, "%zu nodes, %" PRIu64 " leaves", nodes.size(), nl);
    CHECK(lt.too_deep == (deepest_t > kLeafMaxLen), "too_deep %d with the deepest leaf at %u", (int)lt.too_deep, deepest_t);
    if (!lt.too_deep) CHECK(lt.n() == nl && lt.max_len == deepest_t && pl == pt, "table: %" PRIu64 " leaves, deepest %u, payload at %" PRIu64, lt.n(), lt.max_len, pl);
    else CHECK(pl == 8, "a table that is too deep leaves the position where it was");
    cnt.good++;
    cnt.deep += lt.too_deep;
    if (keys_file == "-") return;
    CHECK(nl == leaves && deepest_t == deepest && pt == payload, "%" PRIu64 " leaves, deepest %u, payload at %" PRIu64 "; built with %" PRIu64 ", %u, %" PRIu64, nl, deepest_t, pt, leaves,
          deepest, payload);
    std::vector<uint8_t> kb;
    CHECK(read_file(dir + "/" + keys_file, kb) && kb.size() == nsyms * 4, "keys file");
    for (uint64_t i = 0; i < nsyms; i++) {
        uint32_t want;
        memcpy(&want, kb.data() + 4 * i, 4);
        CHECK(got[i] == want, "symbol %" PRIu64 ": key %u, the payload's leaf holds %u", i, got[i], want);
    }
    cnt.deepest = deepest_t > cnt.deepest ? deepest_t : cnt.deepest;
    cnt.most_leaves = nl > cnt.most_leaves ? nl : cnt.most_leaves;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    std::ifstream man(dir + "/manifest.txt");
    if (!man) { fprintf(stderr, "no manifest in %s\n", dir.c_str()); return 2; }
    Counts cnt;
    std::string line;
    int lines = 0;
    while (std::getline(man, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string file, keys;
        int kind = 0, verdict = 0;
        uint64_t nsyms = 0, leaves = 0, payload = 0;
        uint32_t deepest = 0;
        if (!(in >> file >> kind >> nsyms >> leaves >> deepest >> payload >> verdict >> keys)) { printf("FAIL manifest line: %s\n", line.c_str()); g_fail++; continue; }
        check(dir, file, kind, nsyms, leaves, deepest, payload, verdict, keys, cnt);
        lines++;
    }
    printf("constants: kLeafMaxLen %u\n", kLeafMaxLen);
    printf("%d streams: %d good (%d too deep for the table, the deepest leaf at %u, up to %" PRIu64 " leaves), %d refused, %d failures\n", lines, cnt.good, cnt.deep,
           cnt.deepest, cnt.most_leaves, cnt.refused, g_fail);
    return g_fail ? 1 : 0;
}
