// Stand-alone check of the outage file's reader and of the time-to-epoch conversion
// (gs_read_outages, gs_outage_epochs; gs_host.cpp) for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/outages_file_check.cpp dst-libp2p-test-node_amd/csrc/gs_host.cpp -o outages_file_check
//   ./outages_file_check /tmp/dir        (prints "ok")
// Random outage lists written with comments, blank lines, long lines and two or three columns,
// read back into arrays of exactly the rows' size (a write past them is the sanitizer's to find)
// and under every smaller cap; converted in arrays of their own and in place, against the
// definition applied heartbeat by heartbeat; malformed lines, times at the ends of uint64.
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

static void put(const std::string& path, const std::string& text) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) { fails++; return; }
  fwrite(text.data(), 1, text.size(), f);
  fclose(f);
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string path = dir + "/outages_check.txt";
  uint64_t s = 24680;
  auto rnd = [&]() { return (uint32_t)((s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  gs_config cfg;
  gs_config_default(&cfg);
  for (int round = 0; round < 24; round++) {
    cfg.heartbeat_ns = 1 + rnd() % 1000;
    cfg.hb_phase_ns = rnd() % 5000;
    const uint64_t n = round == 1 ? 0 : 1 + rnd() % 60;
    std::vector<uint32_t> peer(n);
    std::vector<uint64_t> down(n), up(n);
    std::string text = "# outages of round " + std::to_string(round) + "\n";
    for (uint64_t i = 0; i < n; i++) {
      peer[i] = rnd() % 5 == 0 ? 0xFFFFFFFFu : rnd() % 1000;
      down[i] = rnd() % 40000;
      up[i] = rnd() % 7 == 0 ? UINT64_MAX : down[i] + rnd() % 3000;
      if (rnd() % 4 == 0) text += "\n";
      if (rnd() % 6 == 0) text += std::string(1 + rnd() % 3000, ' ');  // (longer than any fixed line buffer)
      text += std::to_string(peer[i]) + (rnd() % 2 ? " " : "\t") + std::to_string(down[i]);
      if (up[i] != UINT64_MAX || rnd() % 2) text += " " + std::to_string(up[i]);
      text += rnd() % 3 == 0 ? "   # restarted\n" : "\n";
    }
    put(path, text);
    uint64_t rows = 99;
    CHECK(gs_read_outages(path.c_str(), nullptr, nullptr, nullptr, 0, &rows) == (n ? GS_ERANGE : GS_OK) && rows == n);
    for (uint64_t cap = 0; cap <= n; cap += 1 + cap / 3) {
      std::vector<uint32_t> p(cap);
      std::vector<uint64_t> d(cap), u(cap);
      uint64_t m = 0;
      const gs_status st = gs_read_outages(path.c_str(), p.data(), d.data(), u.data(), cap, &m);
      CHECK(st == (cap < n ? GS_ERANGE : GS_OK) && m == n);
      for (uint64_t i = 0; i < cap && i < n; i++) CHECK(p[i] == peer[i] && d[i] == down[i] && u[i] == up[i]);
    }
    // the conversion against the definition: epoch h >= 1 is offline iff down <= phase + h * hb < up
    std::vector<uint32_t> po(n), hf(n), ht(n);
    uint64_t kept = 99;
    CHECK(gs_outage_epochs(&cfg, n, peer.data(), down.data(), up.data(), po.data(), hf.data(), ht.data(), &kept) == GS_OK);
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++) {
      uint64_t first = 0, last = 0;
      const uint64_t top = (45000 - cfg.hb_phase_ns) / cfg.heartbeat_ns + 2;
      for (uint64_t h = 1; h <= top; h++) {
        const uint64_t t = cfg.hb_phase_ns + h * cfg.heartbeat_ns;
        if (down[i] <= t && t < up[i]) {
          if (!first) first = h;
          last = h;
        }
      }
      if (!first) continue;
      CHECK(k < kept && po[k] == peer[i] && hf[k] == first);
      if (k < kept) CHECK(up[i] == UINT64_MAX ? ht[k] == GS_OUTAGE_FOREVER : ht[k] == last + 1);
      k++;
    }
    CHECK(k == kept);
    std::vector<uint32_t> ip = peer, ia(n), ib(n);  // in place: the kept peers over the input's
    uint64_t kept2 = 0;
    CHECK(gs_outage_epochs(&cfg, n, ip.data(), down.data(), up.data(), ip.data(), ia.data(), ib.data(), &kept2) == GS_OK);
    CHECK(kept2 == kept);
    for (uint64_t i = 0; i < kept && i < kept2; i++) CHECK(ip[i] == po[i] && ia[i] == hf[i] && ib[i] == ht[i]);
  }
  // malformed lines name themselves; the ends of the number ranges
  const char* bad[] = {"7\n", "1 2 3 4\n", "x 1 2\n", "1 -5 9\n", "4294967296 1 2\n", "1 2 18446744073709551616\n",
                       "1 2x 3\n", "1 2 3x\n", "1 99999999999999999999999999 3\n"};
  for (const char* b : bad) {
    put(path, std::string("0 1 2\n# c\n") + b + "5 6 7\n");
    uint32_t p[4];
    uint64_t d[4], u[4], m = 0;
    CHECK(gs_read_outages(path.c_str(), p, d, u, 4, &m) == GS_EINVAL && m == 3);
  }
  put(path, "4294967295 18446744073709551615 18446744073709551615\n0 0 0");  // (no newline at the end)
  {
    uint32_t p[2];
    uint64_t d[2], u[2], m = 0;
    CHECK(gs_read_outages(path.c_str(), p, d, u, 2, &m) == GS_OK && m == 2 && p[0] == 0xFFFFFFFFu &&
          d[0] == UINT64_MAX && u[0] == UINT64_MAX && p[1] == 0 && d[1] == 0 && u[1] == 0);
    uint32_t a[2], b[2];
    uint64_t kept = 9;
    cfg.heartbeat_ns = 1;
    cfg.hb_phase_ns = 0;
    CHECK(gs_outage_epochs(&cfg, 2, p, d, u, p, a, b, &kept) == GS_ERANGE);  // down at epoch 2^64 - 1
    cfg.heartbeat_ns = UINT64_MAX;
    CHECK(gs_outage_epochs(&cfg, 2, p, d, u, p, a, b, &kept) == GS_OK && kept == 1 && a[0] == 1 && b[0] == GS_OUTAGE_FOREVER);
    cfg.hb_phase_ns = UINT64_MAX;
    d[0] = 5;
    CHECK(gs_outage_epochs(&cfg, 1, p, d, u, p, a, b, &kept) == GS_OK && kept == 1 && a[0] == 1);
    u[0] = 4;
    CHECK(gs_outage_epochs(&cfg, 1, p, d, u, p, a, b, &kept) == GS_EINVAL);
    cfg.heartbeat_ns = 0;
    CHECK(gs_outage_epochs(&cfg, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &kept) == GS_EINVAL);
    cfg.heartbeat_ns = 3;
    CHECK(gs_outage_epochs(&cfg, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &kept) == GS_OK && kept == 0);
    CHECK(gs_outage_epochs(&cfg, 1, p, d, u, nullptr, a, b, &kept) == GS_EINVAL);
    CHECK(gs_outage_epochs(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &kept) == GS_EINVAL);
  }
  uint64_t m = 7;
  CHECK(gs_read_outages((dir + "/missing").c_str(), nullptr, nullptr, nullptr, 0, &m) == GS_EINVAL && m == 0);
  CHECK(gs_read_outages(path.c_str(), nullptr, nullptr, nullptr, 0, nullptr) == GS_EINVAL);
  CHECK(gs_read_outages(nullptr, nullptr, nullptr, nullptr, 0, &m) == GS_EINVAL);
  remove(path.c_str());
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
