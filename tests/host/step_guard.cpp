// Test helper: runs the guard of vrt_hip_transmittance_step (csrc/vrt_step_guard.hpp, host-only) over rows "s0,s1,... delta n" given
// as arguments -- sample points separated by commas, "-" for an empty list, in strtof's notation (inf, nan, hexadecimal floats) -- and
// prints one line per row: "accept <steps> <work>" or "refuse <reason number> <message>".  Runs no loop and needs no library or GPU.
// tests/test_query_scenes.py replays the float32 loop for the accepted rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vrt_step_guard.hpp"

int main(int argc, char **argv)
{
    if (argc < 4 || (argc - 1) % 3) return 2;
    for (int a = 1; a + 2 < argc; a += 3) {
        std::vector<float> s;
        if (strcmp(argv[a], "-"))
            for (const char *p = argv[a]; *p;) {
                char *end;
                s.push_back(strtof(p, &end));
                if (end == p) return 2;
                p = *end == ',' ? end + 1 : end;
            }
        const float delta = strtof(argv[a + 1], nullptr);
        const unsigned long n = strtoul(argv[a + 2], nullptr, 10);
        const vrtk::StepGuard g = vrtk::step_guard(s.data(), s.size(), delta, (uint32_t)n);
        if (g.refusal) printf("refuse %d %s\n", g.refusal, vrtk::step_refusal_message(g.refusal));
        else printf("accept %llu %llu\n", (unsigned long long)g.steps, (unsigned long long)g.work);
    }
    return 0;
}
