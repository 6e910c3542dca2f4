// Stand-alone check of the dial list's text file (gs_read_dials / gs_write_dials, gs_host.cpp)
// for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/dials_file_check.cpp dst-libp2p-test-node_amd/csrc/gs_host.cpp -o dials_file_check
//   ./dials_file_check /tmp/dir        (prints "ok")
// Round trips of random graphs, the cap contract with buffers of exactly cap entries (a write
// past them is the sanitizer's to find), long lines, a file without a final newline, malformed rows.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/gossipsim.h"

static int fails = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      fprintf(stderr, "line %d: %s\n", __LINE__, #x);              \
      fails++;                                                     \
    }                                                              \
  } while (0)

static void put(const std::string& path, const std::string& text) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) { perror(path.c_str()); exit(2); }
  fwrite(text.data(), 1, text.size(), f);
  fclose(f);
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string path = dir + "/dials_check.txt";
  uint64_t s = 12345;
  auto rnd = [&]() { return (uint32_t)((s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  for (int round = 0; round < 20; round++) {
    const uint32_t N = 2 + rnd() % 200;
    // a random CSR: entry (u, w) for u < w with probability ~ 1/8, flags at random
    std::vector<std::vector<std::pair<uint32_t, uint8_t>>> adj(N);
    for (uint32_t u = 0; u < N; u++)
      for (uint32_t w = u + 1; w < N; w++)
        if (rnd() % 8 == 0) {
          const uint8_t f = 1 + rnd() % 3;  // u dialed, w dialed, both
          adj[u].push_back({w, (uint8_t)((f & 1) | (rnd() & 2))});
          adj[w].push_back({u, (uint8_t)((f >> 1) | (rnd() & 2))});
        }
    std::vector<uint64_t> row(N + 1, 0);
    std::vector<uint32_t> col, dial_u, dial_w;
    std::vector<uint8_t> flags;
    for (uint32_t u = 0; u < N; u++) {
      for (auto& e : adj[u]) {
        col.push_back(e.first);
        flags.push_back(e.second);
        if (e.second & 1) { dial_u.push_back(u); dial_w.push_back(e.first); }
      }
      row[u + 1] = col.size();
    }
    CHECK(gs_write_dials(path.c_str(), N, row.data(), col.data(), flags.data()) == GS_OK);
    uint64_t n = 99;
    const gs_status st0 = gs_read_dials(path.c_str(), nullptr, nullptr, 0, &n);
    CHECK(n == dial_u.size() && st0 == (n ? GS_ERANGE : GS_OK));
    for (uint64_t cap : {n / 2, n}) {  // buffers of exactly cap entries
      std::vector<uint32_t> d(cap), t(cap);
      uint64_t m = 0;
      const gs_status st = gs_read_dials(path.c_str(), d.data(), t.data(), cap, &m);
      CHECK(m == n && st == (cap < n ? GS_ERANGE : GS_OK));
      for (uint64_t i = 0; i < cap; i++) CHECK(d[i] == dial_u[i] && t[i] == dial_w[i]);
    }
  }
  uint32_t d[4], t[4];
  uint64_t n = 0;
  put(path, "# c\n\n0 1\n 4294967295\t16777215 # x\n7 8");  // no final newline
  CHECK(gs_read_dials(path.c_str(), d, t, 4, &n) == GS_OK && n == 3 && d[1] == 4294967295u && t[1] == 16777215u &&
        d[2] == 7 && t[2] == 8);
  put(path, "1 2 " + std::string(5000, ' ') + "\n3 4\n");  // a line longer than any fixed buffer
  CHECK(gs_read_dials(path.c_str(), d, t, 4, &n) == GS_OK && n == 2 && d[1] == 3);
  put(path, "1 2 #" + std::string(5000, 'x') + "\n3 4\n");  // a long comment is no row
  CHECK(gs_read_dials(path.c_str(), d, t, 4, &n) == GS_OK && n == 2 && d[0] == 1 && t[1] == 4);
  for (const char* bad : {"x 1\n", "1\n", "1 2 3\n", "1 -2\n", "1 4294967296\n", "1 2x\n", "99999999999999999999999 1\n"}) {
    put(path, bad);
    CHECK(gs_read_dials(path.c_str(), d, t, 4, &n) == GS_EINVAL);
  }
  CHECK(gs_read_dials((dir + "/missing").c_str(), d, t, 4, &n) == GS_EINVAL);
  CHECK(gs_read_dials(path.c_str(), d, t, 4, nullptr) == GS_EINVAL);
  CHECK(gs_write_dials(nullptr, 0, nullptr, nullptr, nullptr) == GS_EINVAL);
  remove(path.c_str());
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
