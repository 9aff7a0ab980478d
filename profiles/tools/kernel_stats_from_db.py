"""Per-kernel statistics (calls, total / mean / min / max ns) and the
trainer's dispatches one by one, from the SQLite database that
``rocprofv3 --kernel-trace --stats -d DIR -o NAME -- ...`` writes.

    python profiles/tools/kernel_stats_from_db.py DIR/NAME_results.db OUT.csv
"""

import csv
import sqlite3
import sys


def main(db, out):
    c = sqlite3.connect(db)
    rows = list(c.execute(
        'select name, count(*), sum(duration), avg(duration), min(duration), '
        'max(duration) from kernels group by name order by sum(duration) desc'))
    with open(out, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['kernel', 'calls', 'total_ns', 'mean_ns', 'min_ns',
                    'max_ns'])
        for r in rows:
            w.writerow([r[0], r[1], r[2], round(r[3]), r[4], r[5]])
        w.writerow([])
        w.writerow(['trainer dispatch (in order)', 'grid_x', 'grid_y',
                    'duration_ns'])
        for r in c.execute("select name, grid_x, grid_y, duration from "
                           "kernels where name like '%nb_train%' order by "
                           "start"):
            w.writerow(list(r))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
