// episodes_probe.cpp -- TEST ONLY (tests/test_episodes_host.py): the library's own per-episode state machine
// (csrc/nig_episodes.hpp episode_row, episode_counts, episode_log_layout) on the host.  Plain C++17: built with the host
// compiler, needs no device and no HIP.  Reads cases from stdin until it ends, answers on stdout, numbers in hex:
//   R <T> <B> <K> <ret_f32 0|1> <canary u32> <n_cuts> <cut>...  then T*B pairs "<reward bits> <flag word>", step-major
//       -> per cut one block: rows [0, cut) collected in a first call, rows [cut, T) in a second one, the log's memory between
//          them as the kernel leaves it (carry and count stored and loaded again); record arrays start filled with the canary.
//          Block = one line "count" (B words), K lines "ret" (B 64-bit words), 5*K lines "w<j>" (B words, j-major),
//          one line "carry_ret" (B 64-bit words), 4 lines "carry_w" (B words).
//   C <B> <K> <n_episodes>      -> "<counted pairs (k, i), k < K> <sum of k*B + i over them>"
//   L <B> <K> <ld>              -> the fields of episode_log_layout in declaration order
// Without stdin input (argument "--self") it runs one built-in case and prints a checksum: the stand-alone sanitizer run.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nig_episodes.hpp"

using namespace nig;

struct Log {
    int B, K;
    std::vector<double> ret, carry_ret;
    std::vector<uint32_t> w, count, carry_w;
    Log(int B_, int K_, uint32_t canary) : B(B_), K(K_), ret((size_t)K_ * B_), carry_ret(B_, 0.0), w((size_t)5 * K_ * B_, canary), count(B_, 0u), carry_w((size_t)4 * B_, 0u)
    {
        uint64_t c64 = ((uint64_t)canary << 32) | canary;
        for (auto &r : ret) memcpy(&r, &c64, 8);
    }
};

// what collect_episodes_kernel does for lane i: load the carry, run the rows, store it
static void collect(Log &g, const uint32_t *reward_bits, const uint32_t *flags, int t0, int t1, bool ret_f32)
{
    for (int i = 0; i < g.B; ++i) {
        EpisodeCarry c{g.carry_ret[i], g.carry_w[i], g.carry_w[g.B + i], g.carry_w[2 * g.B + i], g.carry_w[3 * g.B + i]};
        uint32_t count = g.count[i];
        auto store = [&](uint32_t k, const EpisodeRecord &r) {
            const size_t at = (size_t)k * g.B + i, KB = (size_t)g.K * g.B;
            g.ret[at] = r.ret; g.w[at] = r.w0; g.w[KB + at] = r.w1; g.w[2 * KB + at] = r.w2; g.w[3 * KB + at] = r.w3; g.w[4 * KB + at] = r.w4;
        };
        for (int t = t0; t < t1; ++t) {
            float r;
            memcpy(&r, &reward_bits[(size_t)t * g.B + i], 4);
            episode_row(c, count, (uint32_t)g.K, r, flags[(size_t)t * g.B + i], ret_f32, store);
        }
        g.carry_ret[i] = c.ret; g.carry_w[i] = c.viol; g.carry_w[g.B + i] = c.c01; g.carry_w[2 * g.B + i] = c.c23; g.carry_w[3 * g.B + i] = c.su;
        g.count[i] = count;
    }
}

static void print32(const uint32_t *p, int n) { for (int i = 0; i < n; ++i) printf("%s%" PRIx32, i ? " " : "", p[i]); printf("\n"); }
static void print64(const double *p, int n)
{
    for (int i = 0; i < n; ++i) { uint64_t b; memcpy(&b, &p[i], 8); printf("%s%" PRIx64, i ? " " : "", b); }
    printf("\n");
}

static void print_log(const Log &g)
{
    print32(g.count.data(), g.B);
    for (int k = 0; k < g.K; ++k) print64(&g.ret[(size_t)k * g.B], g.B);
    for (int r = 0; r < 5 * g.K; ++r) print32(&g.w[(size_t)r * g.B], g.B);
    print64(g.carry_ret.data(), g.B);
    for (int r = 0; r < 4; ++r) print32(&g.carry_w[(size_t)r * g.B], g.B);
}

static int self_test()
{
    const int T = 37, B = 5, K = 3;
    std::vector<uint32_t> rb((size_t)T * B), fl((size_t)T * B);
    uint32_t s = 12345u;
    std::vector<int> step(B, 0);
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < B; ++i) {
            s = s * 1664525u + 1013904223u;
            const float r = (float)(int)(s >> 20) * 1e-3f - 1.0f;
            memcpy(&rb[(size_t)t * B + i], &r, 4);
            step[i] += 1;
            uint32_t f = ((uint32_t)step[i] << NIG_FLAG_STEP_SHIFT) | ((s >> 8) & 0x707Cu);
            if (((s >> 3) & 7u) == 0u || step[i] == 6) { f |= (s & 1u) ? NIG_FLAG_TERMINATED : NIG_FLAG_TRUNCATED; step[i] = 0; }
            fl[(size_t)t * B + i] = f;
        }
    uint64_t sum = 0;
    for (int cut = 0; cut <= T; cut += 9) {
        Log g(B, K, 0x5A5A5A5Bu);
        collect(g, rb.data(), fl.data(), 0, cut, (cut & 1) != 0);
        collect(g, rb.data(), fl.data(), cut, T, (cut & 1) != 0);
        for (int i = 0; i < B; ++i) sum += g.count[i];
        for (auto x : g.w) sum = sum * 31u + x;
    }
    const nig_episode_log_layout L = episode_log_layout(100, 3, 0);
    printf("self-test ok: checksum %" PRIx64 ", layout bytes %" PRId64 ", counted(257, 5) %d\n", sum, L.bytes, (int)episode_counts(0, 4, 257, 5));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "--self") == 0) return self_test();
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'R') {
            int T, B, K, f32, n_cuts;
            uint32_t canary;
            if (scanf("%d %d %d %d %" SCNx32 " %d", &T, &B, &K, &f32, &canary, &n_cuts) != 6) return 2;
            std::vector<int> cuts(n_cuts);
            for (auto &c : cuts) if (scanf("%d", &c) != 1 || c < 0 || c > T) return 2;
            std::vector<uint32_t> rb((size_t)T * B), fl((size_t)T * B);
            for (size_t j = 0; j < rb.size(); ++j) if (scanf("%" SCNx32 " %" SCNx32, &rb[j], &fl[j]) != 2) return 2;
            for (int cut : cuts) {
                Log g(B, K, canary);
                collect(g, rb.data(), fl.data(), 0, cut, f32 != 0);
                collect(g, rb.data(), fl.data(), cut, T, f32 != 0);
                print_log(g);
            }
        } else if (kind == 'C') {
            long long B, K, n, pairs = 0, sum = 0;
            if (scanf("%lld %lld %lld", &B, &K, &n) != 3) return 2;
            for (long long k = 0; k < K; ++k)
                for (long long i = 0; i < B; ++i)
                    if (episode_counts(k, i, B, n)) { pairs += 1; sum += k * B + i; }
            printf("%lld %lld\n", pairs, sum);
        } else if (kind == 'L') {
            long long B, K, ld;
            if (scanf("%lld %lld %lld", &B, &K, &ld) != 3) return 2;
            const nig_episode_log_layout L = episode_log_layout(B, K, ld);
            printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64, L.batch, L.capacity, L.ld, L.bytes, L.off_ret);
            for (int w = 0; w < 5; ++w) printf(" %" PRId64, L.off_w[w]);
            printf(" %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", L.off_count, L.off_carry_ret, L.off_carry_w, L.off_tally, L.off_scratch);
        } else {
            return 2;
        }
    }
    return 0;
}
