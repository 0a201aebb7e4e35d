"""VGPRs, AGPRs, scratch bytes per lane, static LDS bytes and waves per SIMD of the data-path kernels and the
one-launch decodes: hipcc -Rpass-analysis=kernel-resource-usage on fec_engine.hip
(profiles/r0N_kernel_resources.txt).  --all lists every kernel of the file; --root=DIR reads the sources of
another tree (e.g. the parent commit, git archive'd), for a diff of two lists.  (The kernels size their LDS
at launch; the static figure is 0 for them.)  Other arguments are passed to hipcc (e.g. -DFEC_... variants)."""
import os
import re
import subprocess
import sys

ROOT = os.path.abspath(__file__).rsplit("/tools/", 1)[0]
ROOT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--root=")), ROOT)
ALL = "--all" in sys.argv[1:]
EXTRA = [a for a in sys.argv[1:] if a != "--all" and not a.startswith("--root=")]
sys.path.insert(0, ROOT)
from pquic_amd import build as B  # noqa: E402

B.generate_lens_header()  # fec_engine.hip includes the build-generated bitslice_lens_gen.h
cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
       f"{ROOT}/pquic_amd/csrc/fec_engine.hip", "-o", "/dev/null", f"-I{ROOT}/include", f"-I{ROOT}/pquic_amd/csrc",
       "-Rpass-analysis=kernel-resource-usage"] + EXTRA
out = subprocess.run(cmd, capture_output=True, text=True).stderr
want = re.compile(r"k_rlc_(encode_bs2?|recover_bs2?|recover_rows_fused|encode_rows|encode_sp|decode_small|"
                  r"span_decode_small)<(\d+), (\d+|true|false)>|k_rlc_encode_sc(_rows|_rows_var)?<\d+>")
rec, cur = {}, None
for ln in out.splitlines():
    m = re.search(r"Function Name: (\S+)", ln)
    if m:
        cur = m.group(1)
        rec[cur] = {}
        continue
    for key, pat in (("V", r"VGPRs: (\d+)"), ("A", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                     ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
        m = re.search(pat, ln)
        if m and cur:
            rec[cur][key] = int(m.group(1))
rows = []
for name, v in rec.items():
    dm = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    if ALL or want.search(dm):
        rows.append(f"{dm.split('(')[0]:<45} V{v.get('V')} A{v.get('A', 0)} scratch{v.get('scratch')} "
                    f"lds{v.get('lds')} occ{v.get('occ')}")
print("\n".join(sorted(rows)))
