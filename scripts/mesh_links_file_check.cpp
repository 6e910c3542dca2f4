// Stand-alone check of the mesh link file (gs_write_mesh_links and, reading it back,
// gs_read_dials; gs_host.cpp) for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/mesh_links_file_check.cpp dst-libp2p-test-node_amd/csrc/gs_host.cpp -o mesh_links_file_check
//   ./mesh_links_file_check /tmp/dir        (prints "ok")
// Round trips of random meshes in arrays of exactly peers * GS_MESH_W ids and peers counts (a
// read past them is the sanitizer's to find), with and without counts, rows shuffled, full rows,
// counts above the width, the empty mesh, the reader's cap contract on the written file.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <utility>
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
  const std::string path = dir + "/mesh_links_check.txt";
  uint64_t s = 4321;
  auto rnd = [&]() { return (uint32_t)((s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  for (int round = 0; round < 24; round++) {
    const uint32_t N = 1 + rnd() % 120;
    const uint32_t odds = round % 3 == 0 ? 2 : 12;  // every third mesh is dense: full rows
    std::vector<std::vector<uint32_t>> adj(N);
    std::vector<std::pair<uint32_t, uint32_t>> links;
    for (uint32_t u = 0; u < N && round != 1; u++)  // (round 1: the empty mesh)
      for (uint32_t w = u + 1; w < N; w++)
        if (rnd() % odds == 0 && adj[u].size() < GS_MESH_W && adj[w].size() < GS_MESH_W) {
          adj[u].push_back(w);
          adj[w].push_back(u);
          links.push_back({u, w});
        }
    std::sort(links.begin(), links.end());
    std::vector<uint32_t> mesh((size_t)N * GS_MESH_W, 0xFFFFFFFFu);
    std::vector<uint8_t> cnt(N);
    for (uint32_t u = 0; u < N; u++) {
      if (round & 1)  // slots in any order inside a row
        for (size_t i = adj[u].size(); i > 1; i--) std::swap(adj[u][i - 1], adj[u][rnd() % i]);
      for (size_t j = 0; j < adj[u].size(); j++) mesh[(size_t)u * GS_MESH_W + j] = adj[u][j];
      cnt[u] = (uint8_t)adj[u].size();
    }
    for (int with_count = 0; with_count < 2; with_count++) {
      CHECK(gs_write_mesh_links(path.c_str(), N, mesh.data(), with_count ? cnt.data() : nullptr) == GS_OK);
      uint64_t n = 99;
      const gs_status st0 = gs_read_dials(path.c_str(), nullptr, nullptr, 0, &n);
      CHECK(n == links.size() && st0 == (n ? GS_ERANGE : GS_OK));
      for (uint64_t cap : {n / 2, n}) {  // buffers of exactly cap entries
        std::vector<uint32_t> a(cap), b(cap);
        uint64_t m = 0;
        const gs_status st = gs_read_dials(path.c_str(), a.data(), b.data(), cap, &m);
        CHECK(m == n && st == (cap < n ? GS_ERANGE : GS_OK));
        std::vector<std::pair<uint32_t, uint32_t>> got;
        for (uint64_t i = 0; i < cap; i++) {
          CHECK(a[i] < b[i]);
          got.push_back({a[i], b[i]});
        }
        CHECK(std::is_sorted(got.begin(), got.end(), [](auto& x, auto& y) { return x.first < y.first; }));  // row order
        if (cap == n) {
          std::sort(got.begin(), got.end());
          CHECK(got == links);
        }
      }
    }
    if (N > 2) {  // a count above the width reads the row's GS_MESH_W slots and no more
      cnt[N - 1] = 255;
      CHECK(gs_write_mesh_links(path.c_str(), N, mesh.data(), cnt.data()) == GS_OK);
      uint64_t n = 0;
      gs_read_dials(path.c_str(), nullptr, nullptr, 0, &n);
      CHECK(n == links.size());  // (the last row's links have a > b: none is written from it)
    }
  }
  uint32_t one[GS_MESH_W];
  for (uint32_t j = 0; j < GS_MESH_W; j++) one[j] = j + 1;  // a full row without a terminator, no counts
  CHECK(gs_write_mesh_links(path.c_str(), 1, one, nullptr) == GS_OK);
  uint64_t n = 0;
  CHECK(gs_read_dials(path.c_str(), nullptr, nullptr, 0, &n) == GS_ERANGE && n == GS_MESH_W);
  CHECK(gs_write_mesh_links(path.c_str(), 0, nullptr, nullptr) == GS_OK);
  CHECK(gs_read_dials(path.c_str(), nullptr, nullptr, 0, &n) == GS_OK && n == 0);
  CHECK(gs_write_mesh_links(nullptr, 1, one, nullptr) == GS_EINVAL);
  CHECK(gs_write_mesh_links(path.c_str(), 1, nullptr, nullptr) == GS_EINVAL);
  CHECK(gs_write_mesh_links((dir + "/missing/x").c_str(), 1, one, nullptr) == GS_EINVAL);
  remove(path.c_str());
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
