"""Kernel table of ONE steady-state tracker frame from a ``rocprofv3 --kernel-trace --output-format csv`` run of tools/bench_f2m.py.

Frames are delimited by the map's render (each frame starts with exactly one k_render_splat dispatch); the table covers the dispatches
from the second-to-last render-splat up to the last one, i.e. the last complete frame.

Usage:  python tools/f2m_frame_table.py KERNEL_TRACE_CSV [OUT_MD]
"""
import csv
import sys
from collections import OrderedDict


def main(path, out=None):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    starts = [i for i, r in enumerate(rows) if 'k_render_splat' in r['Kernel_Name']]
    if len(starts) < 2:
        raise SystemExit('fewer than two frames in the trace')
    frame = rows[starts[-2]:starts[-1]]
    agg = OrderedDict()
    for r in frame:
        name = r['Kernel_Name'].replace('(anonymous namespace)::', '').split('(')[0][:90]
        ns = int(r['End_Timestamp']) - int(r['Start_Timestamp'])
        c, t = agg.get(name, (0, 0))
        agg[name] = (c + 1, t + ns)
    span = (int(frame[-1]['End_Timestamp']) - int(frame[0]['Start_Timestamp'])) / 1e3
    busy = sum(t for _, t in agg.values()) / 1e3
    lines = [f'One steady-state f2m frame: {len(frame)} dispatches, {busy:.1f} us of kernel time in a {span:.1f} us span', '',
             '| kernel | calls | total us | share |', '|---|---|---|---|']
    for name, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        lines.append(f'| `{name}` | {c} | {t / 1e3:.1f} | {100 * t / 1e3 / busy:.1f} % |')
    text = '\n'.join(lines) + '\n'
    print(text)
    if out:
        open(out, 'w').write(text)


if __name__ == '__main__':
    main(*sys.argv[1:])
