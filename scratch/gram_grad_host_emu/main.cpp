#include "gram_grad_emu.inc"
#include <cstdio>
#include <random>
// `return` inside a kernel before a later barrier would deadlock the emulation: the kernels only return after their last barrier
int main() {
    std::mt19937_64 rng(1);
    std::uniform_real_distribution<double> u(-1.5, 1.5);
    int fails = 0;
    for (int B : {1, 3}) for (int N : {1, 17, 64, 65, 130}) for (int Q : {1, 10, 23}) for (int pad : {0, 3}) {
        const int ldw = N + pad; const long long ws_ = (long long)(N + 1) * ldw + (pad ? 1 : 0);
        std::vector<double> x((size_t)B * N * Q), gm((size_t)B * Q), al(B), w((size_t)B * ws_, NAN);
        for (auto &v : x) v = 100.0 + u(rng);
        for (auto &v : gm) v = (0.9 + 0.4 * u(rng)) / std::max(1.0, Q / 4.0);
        for (auto &v : al) v = 1.2 + 0.4 * u(rng);
        for (int b = 0; b < B; ++b) for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) w[b * ws_ + (size_t)i * ldw + j] = u(rng);
        std::vector<double> r((size_t)B * N), sx((size_t)B * N * Q), sq((size_t)B * N * Q);
        size_t wsb = dpgp_ard_rbf_gram_grad_batched_workspace_bytes(B, N, Q);
        std::vector<double> ws(wsb / 8 + 1);
        int rc = dpgp_ard_rbf_gram_grad_batched_f64(B, N, Q, x.data(), gm.data(), al.data(), w.data(), ldw, ws_, r.data(), sx.data(), sq.data(), ws.data(), wsb, nullptr);
        double err = 0, big = 0;
        for (int b = 0; b < B; ++b) for (int i = 0; i < N; ++i) {
            double rr = 0; std::vector<double> ax(Q, 0.0), aq(Q, 0.0);
            for (int j = 0; j < N; ++j) {
                double e = 0;
                for (int q = 0; q < Q; ++q) { double d = x[((size_t)b * N + i) * Q + q] - x[((size_t)b * N + j) * Q + q]; e += gm[b * Q + q] * d * d; }
                double g = w[b * ws_ + (size_t)i * ldw + j] * al[b] * std::exp(-0.5 * e);
                rr += g;
                for (int q = 0; q < Q; ++q) { double d = x[((size_t)b * N + i) * Q + q] - x[((size_t)b * N + j) * Q + q]; ax[q] += g * d; aq[q] += g * d * d; }
            }
            err = std::max(err, std::fabs(rr - r[b * N + i])); big = std::max(big, std::fabs(rr));
            for (int q = 0; q < Q; ++q) {
                err = std::max(err, std::fabs(ax[q] - sx[((size_t)b * N + i) * Q + q])); err = std::max(err, std::fabs(aq[q] - sq[((size_t)b * N + i) * Q + q]));
                big = std::max(big, std::max(std::fabs(ax[q]), std::fabs(aq[q])));
            }
        }
        bool ok = rc == 0 && err <= 1e-12 * big;
        if (!ok) ++fails;
        printf("B=%d N=%d Q=%d pad=%d rc=%d err %.2e of %.2e %s\n", B, N, Q, pad, rc, err, big, ok ? "ok" : "FAIL");
    }
    return fails;
}
