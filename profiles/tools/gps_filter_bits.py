"""SHA-256 of what the Gaussian-process series likelihood returns on fixed
inputs, one line per case: the 4 single kernels and the 23 sums of
tests/test_gps_terms.py on the tests' own ``problem()`` at P in (1, 2, C - 1,
C, C + 1, 2 C + 1, 600), C = ``device.GPS_BLOCK``, with n from (1, 63, 64, 65,
130) rotated over P as the device tests' ``SHAPES`` rotate it, and per kernel
one batch of edge rows (every cause of a NaN row, a = 0 of every term and of
all; for the single kernels also a repeated time without any noise, which the
sums leave unspecified and which is therefore not hashed for them).  Run it
from the repository root before and after a change to nb_gps_filter.h or to
the numpy twin and compare the listings:

    python profiles/tools/gps_filter_bits.py > listing.txt
        the device: the bytes of ``from_model``'s output.  The library is the
        one ``nautilus_amd._lib`` loads (NAUTILUS_HIP_LIB selects another
        build).
    python profiles/tools/gps_filter_bits.py --twin [OTHER.py]
        no GPU: ``numpy_from_model`` in float64 and in ``np.longdouble`` (the
        10 value bytes of every number).  With OTHER.py, another version of
        nautilus_amd/likelihoods.py (such as ``git show REV:...`` written to a
        file), both listings come out of this one process, the other
        version's first, then the number of lines that differ.  numpy's exp
        and log may differ between machines: compare twin listings of one
        machine only."""

import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import test_gps_likelihood as one                             # noqa: E402
import test_gps_terms as terms                                # noqa: E402
from nautilus_amd import device, likelihoods                  # noqa: E402

N_ALL = (1, 63, 64, 65, 130)
KERNELS = one.GPS_KERNELS + terms.COMBOS


def name_of(kernel):
    return kernel if isinstance(kernel, str) else '+'.join(kernel)


def problem(p, n, kernel):
    return (one if isinstance(kernel, str) else terms).problem(p, n, kernel)


def edge_rows(kernel, m, h):
    """Copies of m and h with one cause per row from row 0 on: a non-finite
    m, every bad hyper-parameter, a = 0 of every term and of all terms."""
    c = device.GPS_BLOCK
    if isinstance(kernel, str):
        bad = one.BAD_HYPER + (one.BAD_Q if kernel == 'sho' else [])
        zeros = [[0]]
    else:
        bad = terms.bad_hyper(kernel)
        zeros = [[col] for col in terms.columns(kernel)] + \
            [terms.columns(kernel)]
    m, h = m.copy(), h.copy()
    row = 0
    for col in (0, c - 1, c, m.shape[1] - 1):
        for value in (np.nan, np.inf, -np.inf):
            m[row, col] = value
            row += 1
    for col, value in bad:
        h[row, col] = value
        row += 1
    for cols in zeros:
        h[row, cols] = 0.0
        row += 1
    assert row < len(m)
    return m, h


def cases():
    """(label, kernel, t, d, sigma, m, h) of every case."""
    c = device.GPS_BLOCK
    for ik, kernel in enumerate(KERNELS):
        for ip, p in enumerate((1, 2, c - 1, c, c + 1, 2 * c + 1, 600)):
            n = N_ALL[(ip + ik) % 5]
            yield ('%s P=%d n=%d' % (name_of(kernel), p, n), kernel,
                   *problem(p, n, kernel))
        t, d, sigma, m, h = problem(c + 3, 130, kernel)
        yield ('%s edge rows' % name_of(kernel), kernel, t, d, sigma,
               *edge_rows(kernel, m, h))
        if isinstance(kernel, str):
            # the second of the pair of equal times has a zero pivot
            h0 = h.copy()
            h0[::2, 2] = 0.0
            yield ('%s equal times, no noise' % kernel, kernel, t, d, None,
                   m, h0)


def value_bytes(out):
    out = np.ascontiguousarray(out)
    raw = out.view(np.uint8).reshape(len(out), out.itemsize)
    if out.dtype == np.longdouble and out.itemsize > 10:
        raw = raw[:, :10]                        # x87: the rest is padding
    return raw.tobytes()


def listing(cls, twin):
    lines = []
    for label, kernel, t, d, sigma, m, h in cases():
        like = cls(one.identity, t, d, sigma, kernel=kernel, normalised=False)
        if twin:
            outs = [('twin %s' % np.dtype(ty).name,
                     like.numpy_from_model(m, h, dtype=ty))
                    for ty in (np.float64, np.longdouble)]
        else:
            outs = [('device', like.from_model(m, h))]
        for what, out in outs:
            lines.append('%-44s %-16s %s  (%d NaN)' % (
                label, what, hashlib.sha256(value_bytes(out)).hexdigest(),
                int(np.isnan(out).sum())))
    return lines


def other_likelihoods(path):
    """The class of another version of likelihoods.py, inside this package."""
    spec = importlib.util.spec_from_file_location(
        'nautilus_amd.likelihoods_other', path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    return module.GaussianProcessSeriesLikelihood


def main():
    mine = likelihoods.GaussianProcessSeriesLikelihood
    if '--twin' not in sys.argv:
        print('\n'.join(listing(mine, False)))
        return
    rest = sys.argv[sys.argv.index('--twin') + 1:]
    if not rest:
        print('\n'.join(listing(mine, True)))
        return
    old, new = listing(other_likelihoods(rest[0]), True), listing(mine, True)
    print('# %s' % os.path.basename(rest[0]))
    print('\n'.join(old))
    print('# nautilus_amd/likelihoods.py')
    print('\n'.join(new))
    differ = sum(a != b for a, b in zip(old, new)) + abs(len(old) - len(new))
    print('# %d lines, %d differ' % (len(new), differ))
    sys.exit(1 if differ else 0)


if __name__ == '__main__':
    main()
