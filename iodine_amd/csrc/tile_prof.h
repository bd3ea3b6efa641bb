// Phase timing of the tile / weight-gradient kernels (tools/tile_phase_prof.md; build with IODINE_EXTRA_HIPCC_FLAGS=-DIODINE_TILE_PROF),
// device and host half; compiled out of the product library.  Device: thread 0 of every block accumulates the s_memtime deltas
// between phase boundaries and writes them to a per-kernel __device__ buffer [block][8].  Host: tp_report prints their averages.
#pragma once
#ifdef IODINE_TILE_PROF
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

constexpr int TP_MAXBLK = 16384;
#define TP_DECL unsigned long long tp_last = __builtin_amdgcn_s_memtime(); unsigned tp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define TP_STAMP(slot)                                                                      \
    do {                                                                                    \
        const unsigned long long tp_now = __builtin_amdgcn_s_memtime();                     \
        tp_acc[slot] += (unsigned)(tp_now - tp_last);                                       \
        tp_last = tp_now;                                                                   \
    } while (0)
#define TP_FLUSH(buf)                                                                       \
    if (threadIdx.x == 0 && blockIdx.x < TP_MAXBLK)                                         \
        for (int i_ = 0; i_ < 8; ++i_) buf[blockIdx.x * 8 + i_] = tp_acc[i_]

// Waits for the stream, reads nblk (at most TP_MAXBLK) blocks of `symbol` (HIP_SYMBOL(buffer)) from block first_block on - a second
// role's half of a [role][TP_MAXBLK][8] buffer - and prints one line on stderr: the title, the sum of all eight averages, then the
// first n_names phases "name average |".  Averages are per block read; per != 0: per `per` (tiles), and no total.
// Returns what it read, [block][8], for a caller that prints more.
inline std::vector<unsigned> tp_report(hipStream_t st, const void* symbol, int nblk, const char* title, const char* const* names, int n_names,
                                       int first_block = 0, double per = 0)
{
    const int nb = std::min(nblk, TP_MAXBLK);
    std::vector<unsigned> hp((size_t)nb * 8);
    (void)hipStreamSynchronize(st);
    (void)hipMemcpyFromSymbol(hp.data(), symbol, hp.size() * sizeof(unsigned), (size_t)first_block * 8 * sizeof(unsigned));
    const double div = per != 0 ? per : nb;
    double sum[8] = {0}, tot = 0;
    for (int b = 0; b < nb; ++b) for (int i = 0; i < 8; ++i) sum[i] += hp[(size_t)b * 8 + i];
    for (int i = 0; i < 8; ++i) tot += sum[i] / div;
    if (per != 0) fprintf(stderr, "%s:", title);
    else fprintf(stderr, "%s, total %.0f:", title, tot);
    for (int i = 0; i < n_names; ++i) fprintf(stderr, " %s %.0f |", names[i], sum[i] / div);
    fprintf(stderr, "\n");
    return hp;
}
// the title of a report, formatted: tp_title("[x prof] ticks per block (%d tiles)", n).c_str()
__attribute__((format(printf, 1, 2))) inline std::string tp_title(const char* fmt, ...)
{
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}
#else
#define TP_DECL
#define TP_STAMP(slot)
#define TP_FLUSH(buf)
#endif
