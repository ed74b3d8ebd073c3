"""The contact kernel's query code without a GPU: cuts what separation_host_cut.py cuts, with sep_rate_at and
contact_query in place of separation_query, out of csrc/trajectory.hip and csrc/spline_core.h, compiles it for the host with the address and
undefined-behaviour sanitizers into a stand-alone program with its own main (the staging area on the heap, 1 / x where the kernel has its
refined reciprocal), runs it on the random, solved and follower families and on the NaN-rule inputs of tests/contact_ref.py for d = 1, 2, 3,
and compares time, rate and search trips with contact_f64 bit for bit.
CPU only:  python tests/checks/contact_host_cut.py [n]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import contact_ref as cf  # noqa: E402
import separation_host_cut as shc  # noqa: E402
import separation_ref as sr  # noqa: E402

FROM_KERNELS = shc.FROM_KERNELS[:-1] + ("sep_rate_at", "contact_query")
MAIN = r"""
template <int D> int run(size_t n, size_t k, const double *in, const double *q, double *out)
{
    SepLds<D> *L = new SepLds<D>;
    for (size_t first = 0; first < n; first += kTrajProblems) {
        const size_t here = n - first < (size_t)kTrajProblems ? n - first : (size_t)kTrajProblems;
        for (size_t p = 0; p < here; ++p)
            for (int x = 0; x < D; ++x)
                for (int side = 0; side < 2; ++side) {
                    const double *s = in + (((first + p) * D + x) * 2 + side) * 8;
                    Knots kn{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
                    kn.check();
                    stage_eval(side ? L->b[x] : L->a[x], (int)p, kn);
                    (side ? L->Tb[x] : L->Ta[x])[p] = kn.t0 + kn.t1;
                }
        for (size_t p = 0; p < here; ++p)
            for (size_t j = 0; j < k; ++j) {
                const size_t e = (first + p) * k + j;
                double time, rate;
                int trips = 0;
                contact_query<D>(*L, (int)p, q[4 * e], q[4 * e + 1], q[4 * e + 2], q[4 * e + 3], time, rate, trips);
                if (trips < 0 || trips > (2 * D + 1) * 13 * kSepTrips) return 1;      // a search that did not end
                out[3 * e] = time; out[3 * e + 1] = rate; out[3 * e + 2] = (double)trips;
            }
    }
    delete L;
    return 0;
}

int main(int argc, char **argv)
{
    const int d = atoi(argv[1]);
    const size_t n = (size_t)atol(argv[2]), k = (size_t)atol(argv[3]);
    std::vector<double> in(n * d * 16), q(n * k * 4), out(n * k * 3);
    FILE *f = fopen(argv[4], "rb");
    if (!f || fread(in.data(), 8, in.size(), f) != in.size() || fread(q.data(), 8, q.size(), f) != q.size()) return 2;
    fclose(f);
    const int st = d == 1 ? run<1>(n, k, in.data(), q.data(), out.data()) : d == 2 ? run<2>(n, k, in.data(), q.data(), out.data())
                                                                                      : run<3>(n, k, in.data(), q.data(), out.data());
    f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) return 2;
    fclose(f);
    return st;
}
"""


def source():
    core, kernels = open(os.path.join(shc.CSRC, "spline_core.h")).read(), open(os.path.join(shc.CSRC, "trajectory.hip")).read()
    parts = [shc.PRELUDE] + [shc.cut(core, name) for name in shc.FROM_CORE] + ["constexpr int kSepTrips = 64;\n"]
    parts += [shc.cut(kernels, name) for name in FROM_KERNELS]
    return "".join(parts).replace("#pragma nounroll", "").replace("#pragma unroll", "") + MAIN


def inputs(name, n, k, d):
    """(A, B, level, lo, hi, delay) of a family, or the NaN-rule inputs: the random family with one spline, window end, delay or level each
    of a few problems spoilt."""
    if name != "nan":
        return cf.family(name, n, k, d)[:6]
    a, b, level, lo, hi, delay = cf.family("random", n, k, d)[:6]
    a[0][6][1], b[d - 1][7][2], a[d - 1][6][3], b[0][6][8] = 0.0, np.inf, -1.0, np.nan
    lo[4, 2], hi[5, 3], delay[9, 1], delay[9, 2], delay[9, 3] = np.nan, np.nan, np.nan, np.inf, -np.inf
    level[10, 0], level[10, 1], level[10, 2] = np.nan, np.inf, -np.inf
    return a, b, level, lo, hi, delay


def main(n=1024, k=8):
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "cut.cpp"), os.path.join(tmp, "cut")
        open(src, "w").write(source())
        subprocess.check_call(["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", exe, src])
        for d in (1, 2, 3):
            for name in ("random", "solved", "follower", "follower0", "nan"):
                a, b, level, lo, hi, delay = inputs(name, n, k, d)
                splines = np.stack([np.stack([np.stack(v[x], axis=1) for v in (a, b)], axis=1) for x in range(d)], axis=1)      # (n, d, 2, 8)
                queries = np.stack([level, lo, hi, delay], axis=2)
                with open(os.path.join(tmp, "in"), "wb") as f:
                    f.write(np.ascontiguousarray(splines, dtype=np.float64).tobytes())
                    f.write(np.ascontiguousarray(queries, dtype=np.float64).tobytes())
                r = subprocess.run([exe, str(d), str(n), str(k), os.path.join(tmp, "in"), os.path.join(tmp, "out")], capture_output=True, text=True)
                assert r.returncode == 0 and not r.stderr, (name, d, r.returncode, r.stderr[-2000:])
                out = np.fromfile(os.path.join(tmp, "out"), dtype=np.float64).reshape(n, k, 3)
                time, rate, trips, _ = cf.contact_f64(a, b, level, lo, hi, delay)
                same = [np.array_equal(out[:, :, 0].view(np.uint64), time.view(np.uint64)), np.array_equal(out[:, :, 1].view(np.uint64), rate.view(np.uint64)),
                        np.array_equal(out[:, :, 2], trips.astype(np.float64))]
                print("%s d = %d: %d queries, time %s, rate %s, trips %s (mean %.1f, most %d); no sanitizer report"
                      % (name, d, n * k, *("the same bits" if s else "DIFFERS" for s in same), trips.mean(), trips.max()))
                assert all(same), (name, d)


if __name__ == "__main__":
    main(*[int(x) for x in sys.argv[1:]])
