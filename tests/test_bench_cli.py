"""bench.py's command line without a GPU: a plain run is the headline alone, `--full` is what adds the rest."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _help_blocks():
    """option -> its help text, from `bench.py --help`"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks, cur = {}, None
    for ln in r.stdout.splitlines():
        m = re.match(r"^  (--[a-z0-9-]+)", ln)
        if m:
            cur = m.group(1)
            blocks[cur] = ln
        elif cur and ln.startswith("    "):
            blocks[cur] += " " + ln.strip()
    return {k: " ".join(v.split()) for k, v in blocks.items()}


def test_full_option_is_documented_and_the_options_only_it_uses_say_so():
    h = _help_blocks()
    assert "--full" in h and "CPU baseline" in h["--full"] and "roofline" in h["--full"]
    for opt in ("--cpu-steps", "--profile-iters", "--concurrent", "--batch-sizes", "--no-traffic-probe", "--no-configs2", "--no-configs4"):
        assert "--full" in h[opt], opt


def test_full_is_accepted_by_the_launcher_check():
    """--dry-run (the launcher check: it reports the environment and exits before any GPU work) parses --full like any other option"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-run", "--full"], capture_output=True, text=True, timeout=120,
                       cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '"dry_run": true' in r.stdout
