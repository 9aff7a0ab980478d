"""Helpers of draw_blocks_ab.sh: one summary line of a bench JSON line, the
array-by-array comparison of two --dump-outputs directories, the mean of one
counter over the nb_draw_kernel dispatches of a rocprofv3 pass."""
import csv
import glob
import json
import os
import sys

import numpy as np


def line(path, tag):
    d = json.loads(open(path).read().strip().splitlines()[-1])
    share = d.get('roofline', {}).get('time_share', {})
    s = '%s ms_per_step %.4f value %.2f time_share_ms %s' % (
        tag, d['ms_per_step'], d['value'],
        {k: round(v, 3) for k, v in share.items()})
    if 'roofline_draw' in d:
        s += ' roofline_draw.avg_launch_ms %.4f' % (
            d['roofline_draw']['avg_launch_ms'])
    print(s)


def dumps(a, b):
    names = sorted(os.path.basename(f)
                   for f in glob.glob(os.path.join(a, '*.npy')))
    assert names and names == sorted(
        os.path.basename(f) for f in glob.glob(os.path.join(b, '*.npy')))
    ok = True
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        eq = x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
        ok &= eq
        print('%-28s %-16s %s' % (n, x.shape, 'equal' if eq else 'DIFFERENT'))
    print('ALL EQUAL' if ok else 'MISMATCH')


def pmc(d, c, tag):
    fs = glob.glob(d + '/**/*counter_collection.csv', recursive=True)
    if not fs:
        print(tag, c, 'no data')
        return
    vals = [float(r['Counter_Value']) for r in csv.DictReader(open(fs[0]))
            if 'nb_draw_kernel' in r['Kernel_Name'] and r['Counter_Name'] == c]
    print(tag, c, 'launches', len(vals),
          'mean %.6g' % (sum(vals) / max(1, len(vals))))


if __name__ == '__main__':
    dict(line=line, dumps=dumps, pmc=pmc)[sys.argv[1]](*sys.argv[2:])
