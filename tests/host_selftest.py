"""What the tests of the host-only units share: building and running a CPU self-test (font-renderer_amd/host/<name>.cpp, a
rule of csrc/Makefile) and splitting its lines.  Each program is built once per session and run once per argument list;
what a line means is its test module's own business.  A plain helper module, imported like fixtures.py."""
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "font-renderer_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _built(name):
    subprocess.check_call(["make", "-C", CSRC, "../host/" + name], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "font-renderer_amd", "host", name)


@functools.lru_cache(maxsize=None)
def _stdout(name, args):
    run = subprocess.run([_built(name), *args], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr          # a property failed: stderr names the case and the property
    return tuple(run.stdout.splitlines())


def lines(name, *args):
    """stdout of host/<name> <args>, line by line; the program exits with status 0"""
    return list(_stdout(name, args))


def named(name, *args):
    """the lines "<case> <text>" -> {case: text}, in the program's order"""
    return dict(line.split(" ", 1) for line in lines(name, *args))


def cases(name, *args):
    """the lines "<case> <key>=<value> ... [null] | <tail>" of the layer programs -> {case: ({key: value}, whether the word
    null stands before the bar, tail)}"""
    out = {}
    for case, rest in named(name, *args).items():
        head, tail = rest.split(" | ", 1)
        out[case] = (dict(f.split("=", 1) for f in head.split(" ") if "=" in f), "null" in head.split(" "), tail)
    return out
