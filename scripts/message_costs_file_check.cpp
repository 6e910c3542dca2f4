// Stand-alone check of the message cost file (gs_write_message_costs, gs_host.cpp) for a
// sanitizer build on the CPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/message_costs_file_check.cpp dst-libp2p-test-node_amd/csrc/gs_host.cpp -o message_costs_file_check
//   ./message_costs_file_check /tmp/dir        (prints "ok")
// Random schedules (sizes, chunk counts, the three presets, three muxers) in arrays of exactly
// n_msgs entries and n_msgs * GS_MC_COLS counts (a read past them is the sanitizer's to find),
// no message at all, large counts; the file is parsed back and every derived column is
// recomputed here from gs_wire_bytes, gs_wire_packets and gs_control_packets.
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
  const std::string path = dir + "/message_costs_check.tsv";
  uint64_t s = 24680;
  auto rnd = [&]() { return (uint32_t)((s = s * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  typedef unsigned long long ull;
  for (int round = 0; round < 27; round++) {
    gs_config cfg;
    CHECK(gs_config_preset(&cfg, round % 3) == GS_OK);
    cfg.muxer = (round / 3) % 3;
    cfg.signed_msgs = round % 2;
    cfg.fragments = 1 + rnd() % 4;
    const uint64_t M = round == 2 ? 0 : 1 + rnd() % 40;  // (round 2: no message at all)
    std::vector<gs_publish> sched(M);
    std::vector<uint64_t> cnt(M * GS_MC_COLS);
    for (uint64_t i = 0; i < M; i++) {
      sched[i].t_pub_ns = 946684800000000000ull + i * 1000000000ull + rnd();
      sched[i].publisher = rnd() % 1000;
      sched[i].msg_size = 200 + rnd() % 300000;
      sched[i].frags = rnd() % 5;  // 0: cfg.fragments
      sched[i].reserved = 0;
      for (int k = 0; k < GS_MC_COLS; k++) cnt[i * GS_MC_COLS + k] = round % 4 == 3 ? (1ull << 40) + rnd() : rnd() % 5000;
    }
    CHECK(gs_write_message_costs(&cfg, path.c_str(), M ? sched.data() : nullptr, M, M ? cnt.data() : nullptr) == GS_OK);
    FILE* f = fopen(path.c_str(), "r");
    CHECK(f != nullptr);
    if (!f) break;
    char head[512];
    CHECK(fgets(head, sizeof head, f) && head[0] == '#');
    uint64_t ih[3], iw[3], ack = 0;
    gs_control_packets(GS_CTRL_IHAVE, cfg.node, cfg.muxer, &ih[0], &ih[1], &ih[2]);
    gs_control_packets(GS_CTRL_IWANT, cfg.node, cfg.muxer, &iw[0], &iw[1], &iw[2]);
    gs_control_packets(GS_CTRL_ACK, cfg.node, cfg.muxer, &ack, nullptr, nullptr);
    for (uint64_t i = 0; i < M; i++) {
      ull v[19];
      int got = 0;
      for (int k = 0; k < 19; k++) got += fscanf(f, "%llu", &v[k]) == 1;
      CHECK(got == 19);
      const uint64_t* r = &cnt[i * GS_MC_COLS];
      const uint32_t F = sched[i].frags ? sched[i].frags : cfg.fragments;
      CHECK(v[0] == i && v[1] == sched[i].t_pub_ns && v[2] == sched[i].publisher && v[3] == sched[i].msg_size && v[4] == F);
      for (int k = 0; k < GS_MC_COLS; k++) CHECK(v[5 + k] == r[k]);
      const uint64_t payload = sched[i].msg_size / F + (cfg.node == GS_NODE_GO ? 8 : 0);
      const uint64_t W = gs_wire_bytes(payload, cfg.muxer, cfg.signed_msgs);
      uint64_t pk = 0, hd = 0;
      gs_wire_packets(payload, cfg.muxer, cfg.signed_msgs, &pk, &hd);
      CHECK(v[13] == r[GS_MC_DATA_TX] * W + r[GS_MC_IHAVE_TX] * ih[0] + r[GS_MC_IWANT] * iw[0]);
      CHECK(v[14] == r[GS_MC_DATA_RX] * W + r[GS_MC_IHAVE_RX] * ih[0] + r[GS_MC_IWANT] * iw[0]);
      CHECK(v[15] == r[GS_MC_DATA_TX] * pk + r[GS_MC_IHAVE_TX] * ih[1] + r[GS_MC_IWANT] * iw[1]);
      CHECK(v[16] == r[GS_MC_DATA_RX] * pk + r[GS_MC_IHAVE_RX] * ih[1] + r[GS_MC_IWANT] * iw[1]);
      const uint64_t acks = r[GS_MC_DATA_RX] * ((pk + 1) / 2) + r[GS_MC_IHAVE_RX] * ((ih[1] + 1) / 2) +
                            r[GS_MC_IWANT] * ((iw[1] + 1) / 2);
      CHECK(v[17] == acks && v[18] == acks * ack);
    }
    int c;
    while ((c = fgetc(f)) == '\n') {}
    CHECK(c == EOF);
    fclose(f);
  }
  gs_config cfg;
  gs_config_preset(&cfg, GS_NODE_RUST);
  const gs_publish one = {946684800000000000ull, 3, 1000, 0, 0};
  const uint64_t cnt1[GS_MC_COLS] = {1, 2, 3, 4, 5, 6, 7, 8};
  CHECK(gs_write_message_costs(nullptr, path.c_str(), &one, 1, cnt1) == GS_EINVAL);
  CHECK(gs_write_message_costs(&cfg, nullptr, &one, 1, cnt1) == GS_EINVAL);
  CHECK(gs_write_message_costs(&cfg, path.c_str(), nullptr, 1, cnt1) == GS_EINVAL);
  CHECK(gs_write_message_costs(&cfg, path.c_str(), &one, 1, nullptr) == GS_EINVAL);
  CHECK(gs_write_message_costs(&cfg, (dir + "/missing/x").c_str(), &one, 1, cnt1) == GS_EINVAL);
  const gs_publish tiny = {946684800000000000ull, 3, 7, 0, 0};  // the rust node needs 8 bytes per fragment
  CHECK(gs_write_message_costs(&cfg, path.c_str(), &tiny, 1, cnt1) == GS_EINVAL);
  remove(path.c_str());
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
