"""Error of the device's emulator scores in units of the fp64 oracle's own
error, case by case (tests/score_cases.py; both against a long double
evaluation of the same networks), and the constant K of
tests/test_score_rows_gpu.py that follows from it: the next power of two at
or above twice the largest ratio.

    python profiles/tools/score_parity.py [OUT]     (default: stdout)

The committed run is profiles/score_parity/ratios.txt."""
import os
import sys

from threadpoolctl import threadpool_limits

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
threadpool_limits(limits=1)         # as tests/conftest.py: the oracle's sums

import accept_cases as ac  # noqa: E402
import score_cases as sc  # noqa: E402
import test_score_rows_gpu as t  # noqa: E402


def main(out):
    cases = ([('per_dim', d) for d in ac.DIMS] +
             [('width',) + de for de in sc.WIDTH] +
             [('periodic', d) for d in sc.PERIODIC])
    out.write('# e_dev / e_ref per case and neural bound m; r2 relative, '
              'score absolute, against ld_scores\n'
              '# %-16s m  %10s %10s %7s   %10s %10s %7s\n' % (
                  'case', 'r2 dev', 'r2 oracle', 'ratio', 'score dev',
                  'oracle', 'ratio'))
    worst = 0.0
    for case in cases:
        name = getattr(sc, case[0])(*case[1:]).name
        for m, (e_dev, e_ref) in enumerate(t.ratios(*case)):
            r = [dev / ref for dev, ref in zip(e_dev, e_ref)]
            worst = max(worst, *r)
            out.write('%-18s %d  %10.3e %10.3e %7.2f   %10.3e %10.3e %7.2f\n'
                      % (name, m, e_dev[0], e_ref[0], r[0], e_dev[1],
                         e_ref[1], r[1]))
    k = 1
    while k < 2.0 * worst:
        k *= 2
    out.write('# largest ratio %.2f -> K = %d (next power of two at or above '
              'twice it)\n' % (worst, k))


if __name__ == '__main__':
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            main(f)
    else:
        main(sys.stdout)
