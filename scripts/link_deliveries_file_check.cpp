// Stand-alone check of the link delivery file (gs_write_link_deliveries, gs_host.cpp) for a
// sanitizer build on the CPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/link_deliveries_file_check.cpp dst-libp2p-test-node_amd/csrc/gs_host.cpp -o link_deliveries_file_check
//   ./link_deliveries_file_check /tmp/dir        (prints "ok")
// Random CSRs with empty rows in arrays of exactly peers + 1, nnz and nnz * GS_LD_COLS entries
// (a read past them is the sanitizer's to find), sparse and dense counts, the largest value,
// a graph without entries; the file is parsed back and compared line by line.
#include <stdio.h>
#include <stdlib.h>

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

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string path = dir + "/link_deliveries_check.txt";
  uint64_t s = 97531;
  auto rnd = [&]() { return (uint32_t)((s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  for (int round = 0; round < 24; round++) {
    const uint32_t N = 1 + rnd() % 90;
    std::vector<uint64_t> row(N + 1, 0);
    std::vector<uint32_t> col;
    for (uint32_t u = 0; u < N; u++) {
      const uint32_t deg = round == 1 ? 0 : rnd() % 4 == 0 ? 0 : rnd() % 9;  // (round 1: no entry at all)
      for (uint32_t j = 0; j < deg; j++) col.push_back(rnd() % N);
      row[u + 1] = col.size();
    }
    std::vector<uint64_t> cnt(col.size() * GS_LD_COLS, 0);
    for (size_t i = 0; i < cnt.size(); i++)
      if (rnd() % (round % 2 ? 2 : 7) == 0) cnt[i] = rnd() % 5 == 0 ? UINT64_MAX - rnd() % 3 : rnd() % 1000;
    CHECK(gs_write_link_deliveries(path.c_str(), N, row.data(), col.empty() ? nullptr : col.data(),
                                   cnt.empty() ? nullptr : cnt.data()) == GS_OK);
    FILE* f = fopen(path.c_str(), "r");
    CHECK(f != nullptr);
    if (!f) break;
    for (uint32_t u = 0; u < N; u++)
      for (uint64_t e = row[u]; e < row[u + 1]; e++) {
        const uint64_t* r = &cnt[e * GS_LD_COLS];
        if (!(r[0] | r[1] | r[2])) continue;
        unsigned a = 0, b = 0;
        unsigned long long x = 0, y = 0, z = 0;
        CHECK(fscanf(f, "%u %u %llu %llu %llu\n", &a, &b, &x, &y, &z) == 5);
        CHECK(a == u && b == col[e] && x == r[GS_LD_PUBLISH] && y == r[GS_LD_MESH] && z == r[GS_LD_GOSSIP]);
      }
    CHECK(fgetc(f) == EOF);
    fclose(f);
  }
  const uint64_t row1[2] = {0, 1};
  const uint32_t col1[1] = {0};
  const uint64_t cnt1[GS_LD_COLS] = {1, 2, 3};
  CHECK(gs_write_link_deliveries(nullptr, 1, row1, col1, cnt1) == GS_EINVAL);
  CHECK(gs_write_link_deliveries(path.c_str(), 1, nullptr, col1, cnt1) == GS_EINVAL);
  CHECK(gs_write_link_deliveries(path.c_str(), 1, row1, nullptr, cnt1) == GS_EINVAL);
  CHECK(gs_write_link_deliveries(path.c_str(), 1, row1, col1, nullptr) == GS_EINVAL);
  CHECK(gs_write_link_deliveries((dir + "/missing/x").c_str(), 1, row1, col1, cnt1) == GS_EINVAL);
  remove(path.c_str());
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
