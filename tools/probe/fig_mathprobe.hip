// fig_mathprobe -- the device log/exp routines of the E-steps, called directly (test infrastructure, never shipped).
//
// fig_weights_n (fig_engine_shared.h) and fig_pweights (fig_engine_partial.h) replace the library's log / exp / pow with
// hand-written sequences built on v_rcp_f64 and the frexp builtins.  This program includes the engine headers and calls the
// shipped functions themselves -- fig_weights_n<4> and fig_pweights<2>, the instantiations the E-steps use -- one thread per
// group of arguments, so that tests/test_device_math.py can compare them with a high-precision reference.
//
//   fig_mathprobe <weights.f64> <pweights.f64>
//
// Each file holds raw little-endian doubles.  Output, one line per argument, bit patterns in hex:
//   W <x> <w>            w = exp(0.5 log10 x)                     (fig_weights_n)
//   P <x> <t> <w>        t = ln x, w = 10^t from the rounded t    (fig_pweights)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../figbird_amd/csrc/fig_engine.h"

#define PROBE_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "fig_mathprobe: %s: %s\n", #call, hipGetErrorString(e_)); return 2; } } while (0)

__global__ void probe_weights(const double *x, double *w, long long ngroups) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ngroups) return;
    double px[4], wx[4];
    for (int k = 0; k < 4; k++) px[k] = x[4 * i + k];
    fig_weights_n<4>(px, wx);
    for (int k = 0; k < 4; k++) w[4 * i + k] = wx[k];
}

__global__ void probe_pweights(const double *x, double *t, double *w, long long ngroups) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ngroups) return;
    double px[2], tx[2], wx[2];
    for (int k = 0; k < 2; k++) px[k] = x[2 * i + k];
    fig_pweights<2>(px, tx, wx);
    for (int k = 0; k < 2; k++) { t[2 * i + k] = tx[k]; w[2 * i + k] = wx[k]; }
}

static bool read_doubles(const char *path, std::vector<double> &v) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "fig_mathprobe: cannot open %s\n", path); return false; }
    double buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(double), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    if (v.empty()) { fprintf(stderr, "fig_mathprobe: %s holds no arguments\n", path); return false; }
    return true;
}

static unsigned long long bits(double d) { unsigned long long u; memcpy(&u, &d, 8); return u; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: fig_mathprobe <weights.f64> <pweights.f64>\n"); return 1; }
    std::vector<double> xw, xp;
    if (!read_doubles(argv[1], xw) || !read_doubles(argv[2], xp)) return 1;
    const size_t nw = xw.size(), np = xp.size();
    xw.resize((nw + 3) / 4 * 4, 1.0);                      // whole groups: the padding is computed and not printed
    xp.resize((np + 1) / 2 * 2, 1.0);
    const size_t total = xw.size() + xp.size();
    double *dx = nullptr, *dt = nullptr, *dw = nullptr;
    PROBE_HIP(hipMalloc(&dx, total * sizeof(double)));
    PROBE_HIP(hipMalloc(&dt, total * sizeof(double)));
    PROBE_HIP(hipMalloc(&dw, total * sizeof(double)));
    PROBE_HIP(hipMemcpy(dx, xw.data(), xw.size() * sizeof(double), hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(dx + xw.size(), xp.data(), xp.size() * sizeof(double), hipMemcpyHostToDevice));
    PROBE_HIP(hipMemset(dt, 0xff, total * sizeof(double)));
    PROBE_HIP(hipMemset(dw, 0xff, total * sizeof(double)));
    const long long gw = (long long)(xw.size() / 4), gp = (long long)(xp.size() / 2);
    hipLaunchKernelGGL(probe_weights, dim3((unsigned)((gw + 255) / 256)), dim3(256), 0, 0, dx, dw, gw);
    PROBE_HIP(hipGetLastError());
    hipLaunchKernelGGL(probe_pweights, dim3((unsigned)((gp + 255) / 256)), dim3(256), 0, 0, dx + xw.size(), dt + xw.size(), dw + xw.size(), gp);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipDeviceSynchronize());
    std::vector<double> t(total), w(total);
    PROBE_HIP(hipMemcpy(t.data(), dt, total * sizeof(double), hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(w.data(), dw, total * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nw; i++) printf("W %016llx %016llx\n", bits(xw[i]), bits(w[i]));
    for (size_t i = 0; i < np; i++) printf("P %016llx %016llx %016llx\n", bits(xp[i]), bits(t[xw.size() + i]), bits(w[xw.size() + i]));
    hipFree(dx); hipFree(dt); hipFree(dw);
    return 0;
}
