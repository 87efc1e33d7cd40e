"""A/B of library builds on the latency-bound mip calls, where the host's work per call shows: usage ab_mips.py lib1 lib2 ... ;
each library timed in its own subprocess, 3 interleaved rounds.  Per case: the median over 7 repeats of (200 back-to-back calls +
one synchronize) / 200 in microseconds, and a digest of the output, which must be the same for every library.  The last lines are
the table: per library the median of its rounds, and whether every later library lies within (or below) the spread of the first two."""
import hashlib, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("dxt1 64x64 rgba8 chain (1 pass)", "DXT1", 64, 64, 4), ("dxt1 256x256 rgba8 chain (2 passes)", "DXT1", 256, 256, 4),
         ("etc1 256x256 rgb chain (pyramid + 9 encodes)", "ETC1", 256, 256, 3), ("pyramid 1x16384 rgba8 (3 passes)", None, 1, 16384, 4)]
child = r'''
import hashlib, os, statistics, sys, time, torch
ROOT = %r
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ic_amd_loader
pkg = ic_amd_loader.load_package()
dev = torch.device("cuda:0")
g = torch.Generator(device="cuda"); g.manual_seed(7)
res = []
for name, codec, h, w, comps in %r:
    src = torch.randint(0, 256, (h * w * comps,), dtype=torch.uint8, device=dev, generator=g)
    if codec is None:
        out = torch.zeros((1, pkg.mip_pyramid_size(comps, h, w)[0]), dtype=torch.uint8, device=dev)
        call = lambda: pkg.mip_pyramid_device(src, h, w, comps, out=out)
    else:
        c = getattr(pkg, codec)
        out = torch.zeros((1, pkg.mip_chain_size(c, h, w)[0]), dtype=torch.uint8, device=dev)
        ws = torch.zeros((max(1, pkg.mip_workspace_size(c, comps, h, w)),), dtype=torch.uint8, device=dev)
        call = lambda: pkg.encode_mips_device(c, src, h, w, comps, out=out, workspace=ws)
    for _ in range(100): call()
    torch.cuda.synchronize()
    times = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(200): call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / 200 * 1e6)
    res.append("%%.2f %%s" %% (statistics.median(times), hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:12]))
print(" | ".join(res))
'''
libs = sys.argv[1:]
medians = {lib: [[] for _ in CASES] for lib in libs}
digests = [set() for _ in CASES]
for rnd in range(3):
    for lib in libs:
        env = dict(os.environ, ICAMD_ALLOW_LIB_OVERRIDE="1", ICAMD_LIB_PATH=os.path.join(ROOT, lib))
        r = subprocess.run([sys.executable, "-c", child % (ROOT, CASES)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0 or not r.stdout.strip():
            print("%-30s r%d ERR %s" % (lib, rnd, r.stderr[-300:]), flush=True)
            sys.exit(1)  # nothing more on this device after a failure
        line = r.stdout.strip().splitlines()[-1]
        print("%-30s r%d %s" % (lib, rnd, line), flush=True)
        for k, cell in enumerate(line.split(" | ")):
            medians[lib][k].append(float(cell.split()[0]))
            digests[k].add(cell.split()[1])
print("us per call, median of 3 rounds (min .. max):")
for k, case in enumerate(CASES):
    cells = ["%s %.2f (%.2f .. %.2f)" % (lib, statistics.median(medians[lib][k]), min(medians[lib][k]), max(medians[lib][k])) for lib in libs]
    verdict = ""
    if len(libs) > 2:
        hi = max(statistics.median(medians[lib][k]) for lib in libs[:2])
        verdict = " | later libraries within or below the first two: %s" % all(statistics.median(medians[lib][k]) <= hi for lib in libs[2:])
    print("%-46s %s | outputs %s%s" % (case[0], " | ".join(cells), "identical" if len(digests[k]) == 1 else "DIFFER", verdict))
