// quality_column_main.cpp -- the arithmetic of fig_quality_kernel on the CPU (tests/test_base_quality.py builds this with
// -fsanitize=address,undefined and runs it as a program of its own).  It includes the very function the kernel calls per
// (column, read) pair, fig_quality_add_read of fig_quality.h, and the host's table builder of fig_quality_host.h, reads a case
// from the file named on the command line and prints the plane as the bit patterns of its doubles.
//
// Case file (text; doubles as C99 hex floats):  L / e[0..L) / T[0..25) / n_gaps / per gap: `n n_reads`, then per read
// `o len is_partial aux seq` with o = -2147483648 for a read that was not drawn.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../figbird_amd/csrc/fig_quality.h"
#include "../figbird_amd/csrc/fig_quality_host.h"

// the first two sections of pack_read (fig_pack.h): 2-bit codes, 16 per word, then the N mask, 32 per word
static std::vector<uint32_t> pack(const std::string &s) {
    const int len = (int)s.size(), nw2 = (len + 15) >> 4, nwm = (len + 31) >> 5;
    std::vector<uint32_t> w((size_t)(nw2 + nwm), 0u);
    for (int j = 0; j < len; j++) {
        const int c = s[j] == 'A' ? 0 : s[j] == 'C' ? 1 : s[j] == 'G' ? 2 : s[j] == 'T' ? 3 : 4;
        if (c < 4) w[(size_t)(j >> 4)] |= (uint32_t)c << ((j & 15) * 2);
        else w[(size_t)(nw2 + (j >> 5))] |= 1u << (j & 31);
    }
    return w;
}

static bool next_double(FILE *f, double *v) { char tok[128]; if (fscanf(f, "%127s", tok) != 1) return false; *v = strtod(tok, nullptr); return true; }

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: quality_column <case file>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int L = 0;
    if (fscanf(f, "%d", &L) != 1 || L < 1 || L > FIG_Q_MAXL) return 2;
    std::vector<double> e((size_t)L), ins((size_t)L, 0.0);
    for (int k = 0; k < L; k++) if (!next_double(f, &e[(size_t)k])) return 2;
    fig_model m; memset(&m, 0, sizeof(m));
    m.max_read_length = L; m.error_pos_dist = e.data(); m.in_pos_dist = ins.data(); m.del_pos_dist = ins.data();
    for (int i = 0; i < 25; i++) if (!next_double(f, &m.error_type_probs[i])) return 2;
    std::vector<double> lm((size_t)L), le((size_t)L), lt(16);
    fig_quality_tables_model(&m, lm.data(), le.data(), lt.data());
    int ng = 0;
    if (fscanf(f, "%d", &ng) != 1) return 2;
    for (int g = 0; g < ng; g++) {
        int n = 0, nr = 0;
        if (fscanf(f, "%d %d", &n, &nr) != 2 || n < 0 || nr < 0) return 2;
        struct Read { int o, len, rev; std::vector<uint32_t> w; };
        std::vector<Read> reads;
        for (int r = 0; r < nr; r++) {
            long long o; int len, part, aux; char seq[FIG_Q_MAXL + 8];
            if (fscanf(f, "%lld %d %d %d %207s", &o, &len, &part, &aux, seq) != 5 || (int)strlen(seq) != len) return 2;
            const int32_t o32 = (int32_t)o;
            if (fig_quality_check_placements(&o32, 1) < 0) return 3;                       // the library's bounds check
            reads.push_back(Read{o == INT32_MIN ? 0 : (int)o, o == INT32_MIN ? 0 : len, fig_quality_reversed(part, aux), pack(seq)});   // as the kernel stages it
        }
        for (int x = 0; x < n; x++) {
            double a[4] = {0.0, 0.0, 0.0, 0.0};
            for (const Read &rd : reads)
                fig_quality_add_read(a[0], a[1], a[2], a[3], x, rd.o, rd.len, rd.rev, (const uint32_t *)rd.w.data(), (const double *)lm.data(), (const double *)le.data(), (const double *)lt.data());
            for (int b = 0; b < 4; b++) { uint64_t u; memcpy(&u, &a[b], 8); printf("%016llx%c", (unsigned long long)u, b == 3 ? '\n' : ' '); }
        }
    }
    fclose(f);
    return 0;
}
