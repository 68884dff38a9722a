import json, glob, os, sys
D = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
def calls(r):
    """{call name: (min_ms, max_ms)} of one JSON line"""
    out = {}
    if 'schedules' in r:
        for k, v in r['schedules'].items(): out['shortest_paths/' + k] = (v['call_min_ms'], v['call_max_ms'])
    elif 'call_min_ms' in r: out[r['tool'].replace('_time', '')] = (r['call_min_ms'], r['call_max_ms'])
    elif 'min_ms' in r: out[r['tool'].replace('_time', '')] = (r['min_ms'], r['max_ms'])
    for k, v in r.items():
        if k.endswith('_ms') and isinstance(v, list): out[k[:-3]] = (min(v), max(v))
    return out
bad = 0
print('| configuration | call | parent fastest / slowest ms | new fastest / slowest ms | new fastest <= parent slowest |')
print('|---|---|---|---|---|')
for f in sorted(glob.glob(D + '/*.jsonl')):
    rows = [json.loads(l) for l in open(f) if l.startswith('{')]
    by = {'parent': {}, 'new': {}}
    for r in rows:
        for k, (lo, hi) in calls(r).items():
            a = by[r['lib']].setdefault(k, [lo, hi]); a[0] = min(a[0], lo); a[1] = max(a[1], hi)
    for k in by['parent']:
        p, n = by['parent'][k], by['new'][k]
        ok = n[0] <= p[1]; bad += not ok
        print(f"| {os.path.basename(f)[:-6]} | {k} | {p[0]:.3f} / {p[1]:.3f} | {n[0]:.3f} / {n[1]:.3f} | {'yes' if ok else 'NO'} |")
print('failures', bad)
