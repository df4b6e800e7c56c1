"""Device listings of csrc units as hashes: did a source change alter what a kernel executes?

    python tools/isa_listing.py OUT.json [--keep DIR] SUBSTRING [SUBSTRING ...]
    python tools/isa_listing.py --compare A.json B.json

Compiles every entry of csrc/build.py's SOURCES whose file name contains one of the substrings with build.FLAGS plus
`--cuda-device-only -S`, drops comment-only lines and the per-translation-unit `__hip_cuid_` symbol, and writes per unit the SHA-256 of
the rest and its v_mfma count, per kernel the SHA-256 of its body and hipcc's kernel-resource-usage figures.  Two runs (before / after a
refactor) are compared with --compare: it prints every unit and kernel that only one file has or whose hash or figures differ, and exits
non-zero if there is one; --keep leaves the filtered listings in DIR for a textual diff.  No GPU needed."""
import hashlib
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nope-nerf_amd", "csrc"))
import build  # noqa: E402

FIGURES = {"SGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
           "LDS Size [bytes/block]": "lds"}


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def unit(job, keep):
    src, defines = job
    name = build._obj_name(src, defines)[:-2]
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + build.FLAGS + ["-D" + d for d in defines]
    r = subprocess.run(cmd + ["--cuda-device-only", "-S", os.path.join(build.HERE, src), "-o", "-"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    lines = [l for l in r.stdout.splitlines() if l.strip() and not l.lstrip().startswith(";") and "__hip_cuid_" not in l]
    if keep:
        with open(os.path.join(keep, name + ".s"), "w") as f:
            f.write("\n".join(lines) + "\n")
    kernels, fn = {}, None
    for line in r.stderr.splitlines():      # the remarks: "Function Name: <mangled>", then one figure per line
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = kernels.setdefault(m.group(1), {})
        for label, key in FIGURES.items():
            m = re.search(re.escape(label) + r": (\d+)", line)
            if m and fn is not None:
                fn[key] = int(m.group(1))
    for k, fig in kernels.items():          # the body: from the kernel's label to the end-of-function label behind it
        i = next((n for n, l in enumerate(lines) if l.startswith(k + ":")), None)
        if i is not None:
            j = next(n for n in range(i, len(lines)) if lines[n].startswith(".Lfunc_end"))
            fig["sha256"] = sha(lines[i:j])
            fig["v_mfma"] = sum("v_mfma" in l for l in lines[i:j])
    return name, {"sha256": sha(lines), "lines": len(lines), "v_mfma": sum("v_mfma" in l for l in lines), "kernels": kernels}


def compare(path_a, path_b):
    """Print what differs between two listings; the number of differences."""
    with open(path_a) as f:
        a = json.load(f)
    with open(path_b) as f:
        b = json.load(f)
    diffs = []
    if a["flags"] != b["flags"]:
        diffs.append("flags: %s != %s" % (a["flags"], b["flags"]))

    def walk(what, x, y):      # a unit or a kernel: its own figures, then its kernels
        if x is None or y is None:
            diffs.append("%s: only in %s" % (what, path_b if x is None else path_a))
            return
        for key in sorted((set(x) | set(y)) - {"kernels"}):
            if x.get(key) != y.get(key):
                diffs.append("%s: %s %s != %s" % (what, key, x.get(key), y.get(key)))
        kx, ky = x.get("kernels", {}), y.get("kernels", {})
        for k in sorted(set(kx) | set(ky)):
            walk(what + " " + k, kx.get(k), ky.get(k))

    for u in sorted(set(a["units"]) | set(b["units"])):
        walk(u, a["units"].get(u), b["units"].get(u))
    for d in diffs:
        print(d)
    n_kernels = sum(len(u.get("kernels", {})) for u in a["units"].values())
    print("%d units, %d kernels: %s" % (len(a["units"]), n_kernels, "%d differences" % len(diffs) if diffs else "equal"))
    return len(diffs)


def main(argv):
    if argv and argv[0] == "--compare":
        sys.exit(1 if compare(argv[1], argv[2]) else 0)
    keep = None
    if "--keep" in argv:
        keep = argv.pop(argv.index("--keep") + 1)
        argv.remove("--keep")
        os.makedirs(keep, exist_ok=True)
    out, subs = argv[0], argv[1:]
    jobs = [j for j in build.SOURCES if any(s in j[0] for s in subs)]
    with ThreadPoolExecutor(max_workers=min(build.WORKERS, 16)) as ex:
        units = dict(ex.map(lambda j: unit(j, keep), jobs))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"flags": [a for a in build.FLAGS if not a.startswith("-I")], "units": units}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d units -> %s" % (len(units), out))


if __name__ == "__main__":
    main(sys.argv[1:])
