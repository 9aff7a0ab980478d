"""SHA-256 of what the two geometric queries return on fixed inputs: the
log-likelihoods of ``GaussianLikelihood`` (r2 of a bound without emulators)
and the bytes of ``member_count`` (three overlapping members, one of them a
mixture with a cube dimension), for n_dim 3, 20, 50, 100.  Run it from the
repository root before and after a change to those kernels and compare the
listings:

    python profiles/tools/geom_bits.py > listing.txt

The library is the one ``nautilus_amd._lib`` loads (NAUTILUS_HIP_LIB selects
another build)."""

import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from helpers import upload                                    # noqa: E402
from nautilus_amd.likelihoods import GaussianLikelihood      # noqa: E402
from oracle import bounds_oracle as bo                        # noqa: E402


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def main():
    for d in (3, 20, 50, 100):
        rng = np.random.default_rng(4000 + d)
        a = rng.normal(size=(d, d))
        cov = 0.01 * (a @ a.T / d + np.eye(d))
        like = GaussianLikelihood(0.5 + 0.05 * rng.normal(size=d), cov)
        for n in (1, 1000, 70001):
            x = torch.from_numpy(rng.uniform(size=(n, d))).cuda()
            print('d %3d n %6d  loglike      %s' % (d, n, sha(like(x))))
        centres = 0.5 + rng.normal(size=(3, d)) * (0.1 / np.sqrt(d))
        members = []
        for j in range(3):
            b_mat = np.tril(rng.normal(size=(d, d)) * 0.02) + np.eye(d) * 0.3
            if j < 2:
                members.append(bo.OEllipsoid.from_params(centres[j], b_mat))
            else:
                members.append(bo.OMixture.from_params(
                    np.arange(d) == 0,
                    bo.OEllipsoid.from_params(centres[j, 1:], b_mat[1:, 1:])))
        b = upload(bo.OUnion.from_members(members, unit=False))
        for n in (1, 1000, 70001):
            x = centres[rng.integers(3, size=n)] + rng.normal(size=(n, d)) * (
                0.3 / np.sqrt(d))
            count = b.member_count(torch.from_numpy(x).cuda())
            print('d %3d n %6d  member_count %s  (sum %d)' % (
                d, n, sha(count), int(count.sum())))


if __name__ == '__main__':
    main()
