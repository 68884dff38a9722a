import csv, json, re, sys, collections
import os
D = os.path.dirname(os.path.abspath(__file__))
# old kernel name -> new kernel name (bare names, template arguments dropped where the new kernel is a template)
MAP = {
 'k_sp_keys': 'k_arc_keys<false>', 'k_scc_keys': 'k_arc_keys<true>',
 'k_sp_uniq': 'k_arc_uniq', 'k_scc_uniq': 'k_arc_uniq',
 'k_sp_compact': 'k_arc_compact', 'k_scc_compact': 'k_arc_compact',
 'k_sp_split': 'k_arc_split', 'k_scc_split': 'k_arc_split',
 'k_sp_bounds': 'k_key_bounds<32>', 'k_scc_bounds': 'k_key_bounds<32>', 'k_kc_bounds': 'k_key_bounds<32>',
 'k_pr_bounds': 'k_key_bounds<0>+<32>',
 'k_sp_col': 'k_key_col', 'k_scc_col': 'k_key_col', 'k_kc_col': 'k_key_col', 'k_tc_col': 'k_key_col', 'k_pr_col': 'k_key_col',
 'k_sp_forms': 'k_forms', 'k_scc_forms': 'k_forms',
 'k_sp_form_lists': 'k_form_lists', 'k_scc_form_lists': 'k_form_lists', 'k_pr_lists': 'k_form_lists', 'k_lv_form_lists': 'k_form_lists',
 'k_tc_keys': 'k_edge_keys', 'k_kc_keys': 'k_edge_keys', 'k_tc_mark': 'k_edge_mark', 'k_kc_mark': 'k_edge_mark',
 'k_cc_sizes': 'k_comp_sizes', 'k_scc_sizes': 'k_comp_sizes', 'k_cc_summary': 'k_comp_summary', 'k_scc_summary': 'k_comp_summary',
}
def bare(name):
    m = re.search(r'(k_[A-Za-z0-9_]+)(<[^>]*>)?', name)
    if not m: return name.split('(')[0]
    return m.group(1) + (m.group(2) or '')
def load(path, new):
    c = collections.Counter()
    for row in csv.DictReader(open(path)):
        n = bare(row['Name'])
        base = re.sub(r'<.*', '', n)
        if new:
            if base == 'k_key_bounds': key = 'k_key_bounds'
            elif base == 'k_arc_keys': key = 'k_arc_keys'
            else: key = n
        else:
            key = re.sub(r'<.*', '', MAP[base]) if base in MAP else n
        c[key] += int(row['Calls'])
    return c
ok = True
for tool in ('sp', 'scc', 'tc', 'kcore', 'pagerank', 'cc'):
    a = load(f'{D}/parent_{tool}_kernel_stats.csv', False); b = load(f'{D}/new_{tool}_kernel_stats.csv', True)
    diff = {k: (a.get(k, 0), b.get(k, 0)) for k in set(a) | set(b) if a.get(k, 0) != b.get(k, 0)}
    print(tool, 'kernels', len(b), 'launches parent', sum(a.values()), 'new', sum(b.values()), 'differences', diff)
    ok &= not diff
json.dump(MAP, open(f'{D}/kernel_name_map.json', 'w'), indent=1, sort_keys=True)
print('EQUAL' if ok else 'DIFFERENT')
