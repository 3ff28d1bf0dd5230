#!/usr/bin/env python3
"""Per-kernel comparison of two sets of device assembly files (hipcc
--cuda-device-only -S): for every kernel symbol the instruction stream between
its label and .end_amdhsa_kernel, with comments, assembler directives and
local label names stripped, and the kernel_regs.py resource numbers.
usage: kernel_asm_diff.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...]
Prints one line per kernel: symbol, instruction count, same / different /
removed / new; exit status 1 unless every kernel of both sides is `same`."""
import re
import sys

RES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
       "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(paths):
    out = {}
    for path in paths.split(","):
        s = open(path).read()
        res = {}
        for blk in re.split(r"\n  - \.", s[s.rfind("amdhsa.kernels:"):])[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name:
                res[name.group(1)] = tuple((re.search(r"\." + k + r":\s+(\d+)", blk) or [None, "?"])[1] for k in RES)
        for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)", s, re.M):
            sym = m.group(1)
            start = s.rfind("\n" + sym + ":", 0, m.start())
            end = s.find(".end_amdhsa_kernel", m.start())
            body, labels = [], {}
            for line in s[start:end].split("\n")[2:]:
                line = re.sub(r"\s*(;|//).*$", "", line).strip()
                if not line or line.startswith("."):
                    lab = re.match(r"(\.L\w+):$", line)
                    if lab:  # local labels by order of appearance
                        labels[lab.group(1)] = "L%d" % len(labels)
                        body.append(lab.group(1) + ":")
                    continue
                body.append(line)
            text = "\n".join(body)
            text = re.sub(r"\.L\w+", lambda x: labels.get(x.group(0), "L?"), text)
            n = sum(1 for b in body if not b.endswith(":"))
            out[sym] = (text, n, res.get(sym))
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = 0
for sym in sorted(set(old) | set(new)):
    if sym not in new:
        state, n = "removed", old[sym][1]
    elif sym not in old:
        state, n = "new", new[sym][1]
    else:
        n = new[sym][1]
        same_code, same_res = old[sym][0] == new[sym][0], old[sym][2] == new[sym][2]
        state = "same" if same_code and same_res else "different" + ("" if same_code else " code") + ("" if same_res else " resources")
    bad += state != "same"
    print(sym, n, state)
print("# %d kernels old, %d new, %d not the same" % (len(old), len(new), bad))
sys.exit(1 if bad else 0)
