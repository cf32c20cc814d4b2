// Host-side check of the train-triple membership probes of csrc/kge_sampler_device.h: set_contains_wide<4 / 8 / 16> must answer what
// set_contains answers, for every present key and for absent keys, on tables filled by k_set_insert's rule.  Built and run by
// tests/test_set_probe_host.py with the host side under AddressSanitizer / UBSan: every table is a heap block of exactly its own
// size, so a group load that leaves the table is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kge_sampler_device.h"

using kge::kEmpty;
typedef unsigned long long u64;

struct Table {
    u64* slots;
    u64 mask;
    std::vector<u64> keys;
    explicit Table(u64 n_slots) : mask(n_slots - 1) {
        slots = static_cast<u64*>(aligned_alloc(64, n_slots * sizeof(u64)));
        memset(slots, 0xFF, n_slots * sizeof(u64));
    }
    ~Table() { free(slots); }
    void insert(u64 key) {   // k_set_insert, one thread at a time
        u64 s = kge::mix64(key) & mask;
        for (;;) {
            if (slots[s] == kEmpty) { slots[s] = key; keys.push_back(key); return; }
            if (slots[s] == key) return;
            s = (s + 1) & mask;
        }
    }
};

static u64 g_state = 0x243F6A8885A308D3ull;
static u64 next_random() { return kge::mix64(g_state += 0x9E3779B97F4A7C15ull); }
static u64 random_key() {
    const u64 x = next_random();
    return kge::pack_triple((int64_t)(x & 0xFFFFFF) % 0xFFFFFF, (int64_t)((x >> 24) & 0xFFFF), (int64_t)(x >> 40) % 0xFFFFFF);
}
// a key whose home slot in a table of mask + 1 slots is `home`
static u64 key_with_home(u64 mask, u64 home) {
    for (;;) {
        const u64 k = random_key();
        if ((kge::mix64(k) & mask) == home) return k;
    }
}

static long g_checked = 0, g_failed = 0;
static void check_key(const Table& t, u64 key, const char* what) {
    const bool want = kge::set_contains(t.slots, t.mask, key);
    const bool got[3] = {kge::set_contains_wide<4>(t.slots, t.mask, key), kge::set_contains_wide<8>(t.slots, t.mask, key),
                         kge::set_contains_wide<16>(t.slots, t.mask, key)};
    for (int w = 0; w < 3; ++w) {
        ++g_checked;
        if (got[w] != want) {
            ++g_failed;
            fprintf(stderr, "MISMATCH %s: %llu slots, key %016llx (home %llu): set_contains %d, set_contains_wide<%d> %d\n", what,
                    t.mask + 1, key, kge::mix64(key) & t.mask, (int)want, 4 << w, (int)got[w]);
        }
    }
}
// every present key (must be found), random absent keys, and absent keys of every home slot (the whole run up to its empty slot)
static void check_table(const Table& t, int n_absent, const char* what) {
    for (u64 k : t.keys) {
        if (!kge::set_contains(t.slots, t.mask, k)) { ++g_failed; fprintf(stderr, "%s: inserted key %016llx not found\n", what, k); }
        check_key(t, k, what);
    }
    int done = 0;
    while (done < n_absent) {
        const u64 k = random_key();
        bool present = false;
        for (u64 q : t.keys) present |= q == k;
        if (present) continue;
        check_key(t, k, what);
        ++done;
    }
    const u64 homes = t.mask + 1 < 64 ? t.mask + 1 : 64;
    for (u64 h = 0; h < homes; ++h) {
        const u64 home = (t.mask - h) & t.mask;   // the last slots of the table first
        const u64 k = key_with_home(t.mask, home);
        check_key(t, k, what);
    }
}

int main() {
    {   // 16 slots, 8 keys: the smallest table kernels.triple_set_build makes; a 16-slot group is the whole table
        for (int rep = 0; rep < 32; ++rep) {
            Table t(16);
            while (t.keys.size() < 8) t.insert(random_key());
            check_table(t, 64, "16 slots / 8 random keys");
        }
    }
    {   // 1 024 slots, 512 keys: load 0.5
        Table t(1024);
        while (t.keys.size() < 512) t.insert(random_key());
        check_table(t, 4096, "1024 slots / 512 random keys");
    }
    // every key shares one home slot near the end, so the run wraps past the end of the table: each home of the last group, both sizes
    for (u64 n_slots : {(u64)16, (u64)1024}) {
        for (u64 back = 1; back <= 16; ++back) {
            Table t(n_slots);
            const u64 home = n_slots - back;
            const size_t n_keys = n_slots == 16 ? 8 : 40;
            while (t.keys.size() < n_keys) t.insert(key_with_home(t.mask, home));
            check_table(t, 64, "one home slot, run wraps the end");
            // the run is [home, home + n_keys): its last key sits in the run's last slot, the slot behind it is empty
            const u64 last = (home + n_keys - 1) & t.mask;
            if (t.slots[last] != t.keys.back() || t.slots[(last + 1) & t.mask] != kEmpty) {
                ++g_failed;
                fprintf(stderr, "table construction: run of home %llu does not end where expected\n", home);
            }
        }
    }
    printf("set probe host check: %ld comparisons, %ld failures\n", g_checked, g_failed);
    return g_failed == 0 ? 0 : 1;
}
