"""cost of genotyper --bootstrap 100 at 1 M pairs: batched / T1K_BOOTSTRAP_SERIAL=1 / without the flag, fresh processes alternating,
stopwatch around the process, every run under its own time limit; stops at the first run that does not end well (profiles/boot_cost_1M.log,
DESIGN §16).  python tools/boot_cost.py [rounds [logfile]]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # (tools/ lies one level below the root)
WORK = os.environ.get("T1K_BOOT_COST_DIR", "/tmp/t1k_boot_cost")
os.makedirs(WORK, exist_ok=True)
log = open(sys.argv[2] if len(sys.argv) > 2 else os.path.join(WORK, "boot_cost_1M.log"), "w")


def say(s):
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


synth = os.path.join(ROOT, "tools", "t1k_synth")
geno = os.path.join(ROOT, "t1k_amd", "bin", "genotyper")
ref = os.path.join(WORK, "ref.fa")
with open(ref, "w") as f:
    subprocess.run([synth, "ref-rna", "--genes", "24", "--scale", "1.0", "--seed", "20250614"], check=True, stdout=f, timeout=300)
subprocess.run([synth, "reads", "--ref", ref, "--pairs", "1000000", "--len", "150", "--seed", "2", "--out", os.path.join(WORK, "r")], check=True, timeout=300)
say("input: 24 genes, 1 000 000 pairs of 2 x 150")
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ways = [("plain", [], {}), ("batched", ["--bootstrap", "100"], {}), ("serial", ["--bootstrap", "100"], {"T1K_BOOTSTRAP_SERIAL": "1"})]
times = {w[0]: [] for w in ways}
texts = {}
for rnd in range(rounds):
    for name, extra, env in ways:
        out = os.path.join(WORK, "o_" + name)
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", "170", geno, "-f", ref, "-1", os.path.join(WORK, "r_1.fq"), "-2", os.path.join(WORK, "r_2.fq"), "-o", out, "-t", "16"] + extra,
                           stderr=subprocess.PIPE, text=True, env=dict(os.environ, T1K_DEBUG_PHASES="1", **env))
        dt = time.time() - t0
        if r.returncode != 0:
            say("round %d %s: exit status %d after %.1f s\n%s" % (rnd, name, r.returncode, dt, r.stderr[-3000:]))
            sys.exit(1)
        times[name].append(dt)
        lines = [l for l in r.stderr.splitlines() if "bootstrap:" in l or "quantify:" in l or "EM " in l]
        say("round %d %-8s %.3f s\n  %s" % (rnd, name, dt, "\n  ".join(lines)))
        texts[name] = {k: open(out + k, "rb").read() for k in ("_genotype.tsv", "_allele.tsv")}
        if name != "plain":
            texts[name]["_bootstrap.tsv"] = open(out + "_bootstrap.tsv", "rb").read()
for name in times:
    v = sorted(times[name])
    say("%-8s wall: median %.3f s (min %.3f, max %.3f) over %d" % (name, v[len(v) // 2], v[0], v[-1], len(v)))
say("genotype and allele tables identical in all three: %s" % all(texts[n][k] == texts["plain"][k] for n in texts for k in ("_genotype.tsv", "_allele.tsv")))
say("bootstrap table identical, batched and serial: %s" % (texts["batched"]["_bootstrap.tsv"] == texts["serial"]["_bootstrap.tsv"]))
say("first lines of the table:\n" + "\n".join(texts["batched"]["_bootstrap.tsv"].decode().splitlines()[:12]))
