"""Per-case verdict over three runs of one of the bench tools that print a
median (min, max) per case -- gps_bench.py, gps_terms_bench.py, chi2_bench.py,
fold_bench.py -- in the order parent, new, parent (NAUTILUS_HIP_LIB selects the
parent commit's library):

    python profiles/tools/parent_new_verdict.py PARENT1 NEW PARENT2 [ONLY]

A case is a line `<name> median <us> us (min <us>, max <us>)` that is not
indented (an indented one is a comparison printed under its case); with ONLY, a
regular expression, the cases whose name it matches (the library's own calls
among the compositions they are compared with).  The margin of a case is the
parent's own noise: the larger of the gap between its two medians and its
largest max - min within a run.  The new median may exceed the slower of the
parent's two medians by no more than that."""

import re
import sys

LINE = re.compile(r'^(\S.*?)\s+median\s+([\d.]+) us \(min\s+([\d.]+), '
                  r'max\s+([\d.]+)\)')


def cases(path, only):
    out = {}
    for line in open(path):
        m = LINE.match(line)
        if m and re.search(only, m.group(1)):
            name = ' '.join(m.group(1).split())
            assert name not in out, name
            out[name] = tuple(float(v) for v in m.groups()[1:])
    return out


def main():
    only = sys.argv[4] if len(sys.argv) > 4 else ''
    a, new, b = (cases(path, only) for path in sys.argv[1:4])
    assert list(a) == list(new) == list(b) and a
    width = max(len(case) for case in a)
    print('%-*s %9s %9s %9s %8s %8s  %s' % (
        width, 'case (median us)', 'parent 1', 'new', 'parent 2', 'margin',
        'over', 'verdict'))
    bad = 0
    for case in a:
        gap = abs(a[case][0] - b[case][0])
        spread = max(a[case][2] - a[case][1], b[case][2] - b[case][1])
        margin = max(gap, spread)
        over = new[case][0] - max(a[case][0], b[case][0])
        bad += over > margin
        print('%-*s %9.1f %9.1f %9.1f %8.1f %+8.1f  %s' % (
            width, case, a[case][0], new[case][0], b[case][0], margin, over,
            'within' if over <= margin else 'OUTSIDE'))
    print('%d cases, %d outside the margin' % (len(a), bad))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
