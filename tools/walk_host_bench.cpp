// The CPU baseline of tools/walk_paths.py: TreeIndex::walk_host of the C++ mirror (std::upper_bound
// per node) over a flat tree and a batch of 16-byte queries read from files.
//
//   walk_host_bench DIR THREADS REPS
//
// DIR holds nodes.bin, segments.bin, children.bin, bounds.bin (the flat records), pivot_keys.bin and
// queries.bin (16 bytes per key).  Prints one JSON line: the time of every repetition (host clock,
// the whole call: descents and the CSR lists), and sums of the result for the caller to compare
// with the device's.
#include <turtle_kv_amd/filter_builder.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace turtle_kv_amd;

template <class T>
static std::vector<T> read_all(const std::string& path)
{
  std::vector<T> v;
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path.c_str());
    std::exit(2);
  }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((usize)bytes / sizeof(T));
  if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}

int main(int argc, char** argv)
{
  if (argc != 4) {
    std::fprintf(stderr, "usage: walk_host_bench DIR THREADS REPS\n");
    return 2;
  }
  const std::string dir = argv[1];
  const unsigned threads = (unsigned)std::atoi(argv[2]);
  const int reps = std::atoi(argv[3]);
  const auto key_bytes = read_all<char>(dir + "/pivot_keys.bin");
  std::vector<std::string> pivot_keys;
  for (usize i = 0; i + 16 <= key_bytes.size(); i += 16) pivot_keys.emplace_back(key_bytes.data() + i, 16);
  TreeIndex tree;
  TreeIndex::from_flat(read_all<tkv_amq_tree_node>(dir + "/nodes.bin"),
                       read_all<tkv_amq_tree_segment>(dir + "/segments.bin"),
                       read_all<tkv_amq_tree_child>(dir + "/children.bin"), read_all<u32>(dir + "/bounds.bin"),
                       std::move(pivot_keys), tree);
  const auto q = read_all<char>(dir + "/queries.bin");
  std::vector<std::string_view> items;
  items.reserve(q.size() / 16);
  for (usize i = 0; i + 16 <= q.size(); i += 16) items.emplace_back(q.data() + i, 16);

  std::vector<double> ms;
  unsigned long long entries = 0, leaf_sum = 0, begin_sum = 0;
  for (int r = 0; r < reps; ++r) {
    TreePaths out;
    const auto t0 = std::chrono::steady_clock::now();
    tree.walk_host(items, out, threads);
    const auto t1 = std::chrono::steady_clock::now();
    ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    entries = out.leaf.size();
    leaf_sum = begin_sum = 0;
    for (u32 v : out.leaf) leaf_sum += v;
    for (u32 v : out.begin) begin_sum += v;
  }
  std::vector<double> sorted = ms;
  std::sort(sorted.begin(), sorted.end());
  std::printf("{\"threads\": %u, \"reps\": %d, \"queries\": %zu, \"median_ms\": %.3f, \"min_ms\": %.3f, "
              "\"max_ms\": %.3f, \"entries\": %llu, \"leaf_sum\": %llu, \"begin_sum\": %llu}\n",
              threads, reps, items.size(), sorted[sorted.size() / 2], sorted.front(), sorted.back(), entries, leaf_sum,
              begin_sum);
  return 0;
}
