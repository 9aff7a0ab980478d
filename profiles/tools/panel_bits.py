"""SHA-256 of what the two likelihoods of the panel driver (nb_panel.h) return
on fixed inputs, one line per case: the data-vector likelihood with a full
covariance (nb_chi2.hip) and the folded Poisson likelihood (nb_fold.hip), on
the device tests' own ``problem()`` at every entry of their ``SHAPES``; per
kernel one batch for every block of points its launcher picks (n = 16384 and
32768 rows, 16385 for the folded one) over two panels (P = 257); and per
kernel batches of edge rows: the NaN and +-inf placements of
``test_nan_stays_in_its_row``, the rows of ``test_edge_rows``.  Run it from
the repository root before and after a change to nb_panel.h or to a policy
and compare the listings:

    python profiles/tools/panel_bits.py > listing.txt

The library is the one ``nautilus_amd._lib`` loads (NAUTILUS_HIP_LIB selects
another build).  Every case runs in a child process of its own under a time
limit; the first one that fails ends the run."""

import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import test_data_likelihood_gpu as chi2                       # noqa: E402
import test_folded_poisson_gpu as fold                        # noqa: E402

STEP_SECONDS = 120
CASES = [('chi2', p, n) for p, n in chi2.SHAPES] + \
    [('chi2 rows', 257, 16384), ('chi2 rows', 257, 32768)] + \
    [('chi2 edge', p) for p in (17, 129)] + \
    [('fold',) + shape for shape in fold.SHAPES] + \
    [('fold rows', 257, 33, 16385)] + \
    [('fold edge', p, ks) for p, ks in ((17, 5), (257, 33), (1025, 130))]


def chi2_edge(m, p):
    """Blocks of 40 rows, one per placement of test_nan_stays_in_its_row."""
    blocks = []
    for c_nan, c_inf in ((2, 0), (p - 1, 16), (0, p - 1)):
        dirty = m[:40].copy()
        dirty[5, c_nan] = np.nan
        dirty[19, c_inf] = np.inf
        blocks.append(dirty)
    dirty = m[:40].copy()
    dirty[19, 3] = -np.inf
    return np.concatenate(blocks + [dirty])


def fold_edge(s, ks):
    """The dirty rows of test_edge_rows."""
    dirty = s.copy()
    dirty[3, 0] = 0.0
    dirty[11, 1] = -1e300
    dirty[12, 2] = 1e6
    dirty[40, 0] = np.nan
    dirty[41, ks - 2] = np.inf
    dirty[42, 1] = -np.inf
    dirty[43, ks - 1] = np.nan
    dirty[44, ks - 1] = np.inf
    dirty[45, ks - 1] = -np.inf
    dirty[77, 0] = 0.0
    dirty[77, 3] = np.nan
    dirty[99, 0] = 0.0
    dirty[99, ks - 1] = np.inf
    return dirty


def run(kind, *shape):
    """The bytes the library returns for one case."""
    import torch
    from nautilus_amd import PoissonDataLikelihood, device
    if kind.startswith('chi2'):
        p = shape[0]
        d, _, _, m, w = chi2.problem(p, shape[1] if kind == 'chi2' else 530)
        if kind == 'chi2 rows':
            m = np.tile(m, (-(-shape[1] // len(m)), 1))[:shape[1]]
        elif kind == 'chi2 edge':
            m = chi2_edge(m, p)
        out = device.Chi2Table(d, chol_inv=w).loglike(
            torch.from_numpy(np.array(m)).cuda())    # m is read-only
    else:
        if kind == 'fold edge':
            k, resp, e, b, s = fold._edge_problem(*shape)
            s = fold_edge(s, shape[1])
        else:
            k, resp, e, b, s = fold.problem(*shape)
        like = PoissonDataLikelihood(fold.identity, k, exposure=e,
                                     background=b, response=resp)
        out = like.from_model(torch.from_numpy(np.array(s)).cuda())
    out = out.cpu().numpy()
    return '%s  (%d rows, %d NaN)' % (
        hashlib.sha256(out.tobytes()).hexdigest(), len(out),
        int(np.isnan(out).sum()))


def main():
    for case in CASES:
        label = '%-9s %s' % (case[0], ' '.join(str(v) for v in case[1:]))
        res = subprocess.run(
            [sys.executable, os.path.abspath(__file__), '--case', case[0]] +
            [str(v) for v in case[1:]], stdout=subprocess.PIPE,
            timeout=STEP_SECONDS, text=True)
        if res.returncode != 0:
            sys.exit('case %s ended with status %d' % (label, res.returncode))
        print('%-28s %s' % (label, res.stdout.strip()), flush=True)


if __name__ == '__main__':
    if '--case' in sys.argv:
        i = sys.argv.index('--case')
        print(run(sys.argv[i + 1], *(int(v) for v in sys.argv[i + 2:])))
    else:
        main()
