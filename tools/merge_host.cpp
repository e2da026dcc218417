// The leaf merge on host threads, as the yardstick of tools/merge_leaves.py: the same jobs -- per leaf an older
// run of --older items and a newer run of --newer items, half of whose keys exist in the leaf; KEY-byte keys,
// VALUE-byte values -- merged by std::merge and a compaction loop (the first item of a group of equal keys stands,
// an ADD_I32 is folded with the item behind it), keys and values copied into contiguous output arrays, the jobs
// dealt to --threads threads.  Prints one JSON line: the median, minimum and maximum of --reps timings.
//
//   merge_host --leaves 256 --older 16384 --newer 1024 --key 16 --value 101 --deltas 0 --threads 16 --reps 7
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

struct Ref {  // one item of either run: where its key and its value lie
  const uint8_t *key, *value;
  uint32_t vlen;
};

int main(int argc, char** argv)
{
  uint64_t leaves = 256, n_older = 16384, n_newer = 1024, key = 16, value = 101, deltas = 0, threads = 16, reps = 7;
  for (int i = 1; i + 1 < argc; i += 2) {
    const std::string a = argv[i];
    const uint64_t v = std::strtoull(argv[i + 1], nullptr, 10);
    if (a == "--leaves") leaves = v;
    else if (a == "--older") n_older = v;
    else if (a == "--newer") n_newer = v;
    else if (a == "--key") key = v;
    else if (a == "--value") value = v;
    else if (a == "--deltas") deltas = v;
    else if (a == "--threads") threads = v;
    else if (a == "--reps") reps = v;
  }
  const uint64_t nvalue = deltas ? 5 : value, step = n_older / n_newer;
  // keys: zero bytes, then the leaf and the item's number, big-endian, in the last 16 bytes; older item i is 2i,
  // newer item t is older item step * t + 3 (t even) or the odd number behind it (t odd)
  auto put_key = [&](uint8_t* k, uint64_t leaf, uint64_t x) {
    std::memset(k, 0, key);
    for (int b = 0; b < 8; ++b) {
      k[key - 16 + b] = (uint8_t)(leaf >> (56 - 8 * b));
      k[key - 8 + b] = (uint8_t)(x >> (56 - 8 * b));
    }
  };
  std::vector<uint8_t> okeys(leaves * n_older * key), ovals(leaves * n_older * value, 0x5a);
  std::vector<uint8_t> nkeys(leaves * n_newer * key), nvals(leaves * n_newer * nvalue, 0x3c);
  for (uint64_t l = 0; l < leaves; ++l) {
    for (uint64_t i = 0; i < n_older; ++i) {
      put_key(&okeys[(l * n_older + i) * key], l, 2 * i);
      ovals[(l * n_older + i) * value] = 2;  // WRITE
    }
    for (uint64_t t = 0; t < n_newer; ++t) {
      put_key(&nkeys[(l * n_newer + t) * key], l, 2 * (step * t + 3) + (t & 1));
      nvals[(l * n_newer + t) * nvalue] = deltas ? 3 : 2;  // ADD_I32 or WRITE
    }
  }
  std::vector<uint8_t> out_keys(leaves * (n_older + n_newer) * key), out_vals(leaves * (n_older + n_newer) * value);
  std::vector<uint64_t> out_count(leaves);
  std::vector<double> ms;
  for (uint64_t r = 0; r < reps + 1; ++r) {
    std::atomic<uint64_t> next{0};
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (uint64_t t = 0; t < threads; ++t)
      pool.emplace_back([&] {
        std::vector<Ref> a(n_newer), b(n_older), m(n_newer + n_older);
        for (uint64_t l; (l = next.fetch_add(1)) < leaves;) {
          for (uint64_t i = 0; i < n_newer; ++i)
            a[i] = Ref{&nkeys[(l * n_newer + i) * key], &nvals[(l * n_newer + i) * nvalue], (uint32_t)nvalue};
          for (uint64_t i = 0; i < n_older; ++i)
            b[i] = Ref{&okeys[(l * n_older + i) * key], &ovals[(l * n_older + i) * value], (uint32_t)value};
          std::merge(a.begin(), a.end(), b.begin(), b.end(), m.begin(),
                     [&](const Ref& x, const Ref& y) { return std::memcmp(x.key, y.key, key) < 0; });
          uint8_t* ko = &out_keys[l * (n_older + n_newer) * key];
          uint8_t* vo = &out_vals[l * (n_older + n_newer) * value];
          uint64_t kept = 0;
          for (uint64_t i = 0; i < m.size();) {
            uint64_t e = i + 1;
            while (e < m.size() && std::memcmp(m[e].key, m[i].key, key) == 0) ++e;
            std::memcpy(ko, m[i].key, key);
            ko += key;
            if (e - i > 1 && m[i].value[0] == 3) {  // a delta over the leaf's item: op and sum, 5 bytes
              uint32_t x, y;
              std::memcpy(&x, m[i].value + 1, 4);
              std::memcpy(&y, m[i + 1].value + 1, 4);
              x += m[i + 1].value[0] == 0 ? 0u : y;
              vo[0] = m[i + 1].value[0] == 3 ? 3 : 2;
              std::memcpy(vo + 1, &x, 4);
              vo += 5;
            } else {
              std::memcpy(vo, m[i].value, m[i].vlen);
              vo += m[i].vlen;
            }
            ++kept;
            i = e;
          }
          out_count[l] = kept;
        }
      });
    for (auto& th : pool) th.join();
    const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r) ms.push_back(t);  // (the first pass warms the pages)
  }
  std::sort(ms.begin(), ms.end());
  uint64_t kept = 0;
  for (uint64_t c : out_count) kept += c;
  const uint64_t items = leaves * (n_older + n_newer);
  std::printf("{\"host_threads\": %llu, \"leaves\": %llu, \"items\": %llu, \"kept\": %llu, \"median_ms\": %.3f, "
              "\"min_ms\": %.3f, \"max_ms\": %.3f, \"reps\": %zu, \"gitems_per_s\": %.4f}\n",
              (unsigned long long)threads, (unsigned long long)leaves, (unsigned long long)items,
              (unsigned long long)kept, ms[ms.size() / 2], ms.front(), ms.back(), ms.size(),
              items / ms[ms.size() / 2] / 1e6);
  return kept == leaves * (n_older + n_newer - n_newer / 2) ? 0 : 1;
}
