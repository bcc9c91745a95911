// thrust_seeded_probe.cpp -- TEST INFRASTRUCTURE (built by tests/test_sampling_seed_cpu.py with the Thrust headers of the ROCm install, for
// the host).  The seeded with-replacement stream as the reference's sampler would draw it had it seeded its engine:
// thrust::minstd_rand(s_b), discard(idx), thrust::uniform_int_distribution<int>(0, deg - 1).  Reads "s_b idx deg" triples on stdin and
// prints "s_b idx deg k".
#include <thrust/random/linear_congruential_engine.h>
#include <thrust/random/uniform_int_distribution.h>
#include <cstdint>
#include <cstdio>

int main()
{
    unsigned long long sb, idx;
    int deg;
    while (scanf("%llu %llu %d", &sb, &idx, &deg) == 3) {
        thrust::minstd_rand engine((uint32_t)sb);
        engine.discard(idx);
        thrust::uniform_int_distribution<int> dist(0, deg - 1);
        printf("%llu %llu %d %d\n", sb, idx, deg, (int)dist(engine));
    }
    return 0;
}
