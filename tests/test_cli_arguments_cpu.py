"""CPU: the command lines of the sixteen analysis tools, byte for byte.  tests/cli_arguments.json holds what the tools of the commit
before the shared flag table (csrc/host/mvs_tool.hpp: Flag, parse_flags) answered to a fixed list of command lines -- every flag
without a value, with the empty value, with the values on and beyond its bounds, given twice, beside a second refused flag, an
unknown argument and a path flag without a value; every required flag absent; --help beside garbage; the rules across flags -- and
every built tool must answer the same: exit code, stdout and stderr.  tools/record_cli_arguments.py wrote the file and says how the
cases are made.  Every case ends before a DB, a hash file or a device is touched (the DB is the folder nodb/, which is not there);
the tools run in their own folder as ./<tool>, so the usage text is the same everywhere.  No device needed."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")

with open(os.path.join(ROOT, "tests", "cli_arguments.json")) as _f:
    RECORDS = json.load(_f)
TOOLS = sorted({r["tool"] for r in RECORDS})


def answer(record):
    r = subprocess.run(["./" + record["tool"]] + record["argv"], cwd=BIN, capture_output=True, stdin=subprocess.DEVNULL, env=NO_GPU)
    return r.returncode, r.stdout.decode("utf-8", "surrogateescape"), r.stderr.decode("utf-8", "surrogateescape")


def test_the_record_covers_the_sixteen_tools():
    assert len(TOOLS) == 16 and len(RECORDS) >= 300
    assert not os.path.exists(os.path.join(BIN, "nodb"))


@pytest.mark.parametrize("tool", TOOLS)
def test_every_recorded_command_line_is_answered_as_before(tool):
    records = [r for r in RECORDS if r["tool"] == tool]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        answers = list(pool.map(answer, records))
    wrong = []
    for r, got in zip(records, answers):
        want = (r["exit"], r["stdout"], r["stderr"])
        if got != want:
            wrong.append("%s %r\n  recorded %r\n  now      %r" % (tool, r["argv"], want, got))
    assert not wrong, "%d of %d command lines differ:\n%s" % (len(wrong), len(records), "\n".join(wrong))
