"""Per-case verdict over three runs of gps_bench.py or gps_terms_bench.py in
the order parent, new, parent (NAUTILUS_HIP_LIB selects the parent commit's
library):

    python profiles/tools/gps_filter_verdict.py PARENT1 NEW PARENT2

A case is a line with the median (min, max) of nb_gps_loglike.  The margin of
a case is the parent's own noise: the larger of the gap between its two
medians and its largest max - min within a run.  The new median may exceed
the slower of the parent's two medians by no more than that."""

import re
import sys

LINE = re.compile(r'^(P=\d+ n=\d+ \S+)\s+(?:nb_gps_loglike )?median\s+([\d.]+) '
                  r'us \(min\s+([\d.]+), max\s+([\d.]+)\)')


def cases(path):
    out = {}
    for line in open(path):
        m = LINE.match(line)
        if m:
            out[m.group(1)] = tuple(float(v) for v in m.groups()[1:])
    return out


def main():
    a, new, b = (cases(path) for path in sys.argv[1:4])
    assert list(a) == list(new) == list(b) and a
    print('%-40s %9s %9s %9s %8s %8s  %s' % (
        'case (median us)', 'parent 1', 'new', 'parent 2', 'margin', 'over',
        'verdict'))
    bad = 0
    for case in a:
        gap = abs(a[case][0] - b[case][0])
        spread = max(a[case][2] - a[case][1], b[case][2] - b[case][1])
        margin = max(gap, spread)
        over = new[case][0] - max(a[case][0], b[case][0])
        bad += over > margin
        print('%-40s %9.1f %9.1f %9.1f %8.1f %+8.1f  %s' % (
            case, a[case][0], new[case][0], b[case][0], margin, over,
            'within' if over <= margin else 'OUTSIDE'))
    print('%d cases, %d outside the margin' % (len(a), bad))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
