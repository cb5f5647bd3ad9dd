"""csrc/upconv.hip compiled for gfx950 (device side only, nothing runs): upconv_xy, both instantiations, must hold its x-pass
row in flight without scratch -- no VGPR spill, no scratch, two waves per SIMD (the occupancy its 79 KB of LDS allow anyway)."""
import os
import re
import subprocess

from streammos_amd import build


def test_upconv_xy_compiles_without_scratch_or_spills(tmp_path):
    src = os.path.join(os.path.dirname(build.__file__), "csrc", "upconv.hip")
    flags = [f for f in build.FLAGS if f not in ("-fPIC", "-Wall")]
    out = subprocess.run([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", src, "-o",
                                                  str(tmp_path / "upconv.s")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    facts, name = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            facts[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            facts[name][m.group(1).strip()] = int(m.group(2))
    xy = {k: v for k, v in facts.items() if "upconv_xy" in k}
    assert len(xy) == 2, sorted(facts)
    for k, v in xy.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 256 and v["Occupancy"] >= 2, (k, v)
