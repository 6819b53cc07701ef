"""CPU: tests/stream_matrix.py against the sources and against itself.

* Every case id of tests/memory_matrix.py is in the table, with the family and the row it has there.
* Census: `current_stream()` counted per file of twisterl_amd/csrc and per enclosing function equals what the table declares -- a pull
  request that adds a user of the library's stream has to touch the table, and with it say which entry point reaches the new user and
  which case runs it.  The scan looks for this one word and for the line a function starts on.
* Every entry point the table names is a symbol of the C ABI; every one that is not a hook without a delay (`UNLISTED`) or the
  multi-rank broadcast is reached by a case; every case names entry points the GPU test delays (`LISTED`).
* The Python side: `_lib.library_stream` refuses what is no stream, and INTEGRATION.md names the two GPU files.
"""
import glob
import os
import re

import pytest

from tests import memory_matrix as mm
from tests import stream_matrix as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twisterl_amd", "csrc")
WORD = "current_stream()"
# a function starts on a line at column 0 that is no comment, directive, closing brace, namespace / struct / template line, and has a `(`
FUNCTION = re.compile(r"^(?![ \t/#}])(?!namespace|using|template|struct|class|typedef)[^;=]*?\b(\w+)\s*\(")


def count_stream_users(csrc=CSRC):
    """-> {file: {enclosing function: how often the word stands in it}} over every file of `csrc`, files without it left out."""
    out = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        fn, users = None, {}
        for line in open(path, errors="ignore").read().split("\n"):
            m = FUNCTION.match(line)
            if m:
                fn = m.group(1)
            if line.count(WORD):
                users[fn] = users.get(fn, 0) + line.count(WORD)
        if users:
            out[os.path.basename(path)] = users
    return out


def test_every_memory_matrix_case_is_in_the_table():
    assert st.IDS[:len(mm.IDS)] == mm.IDS and len(set(st.IDS)) == len(st.IDS)
    for c in mm.CASES:
        s = st.BY_ID[c.id]
        assert (s.family, s.ref) == (c.family, c.ref) and st.MODE1 in s.modes
        assert (st.MODE2 in s.modes) == (c.family in st.MODE2_FAMILIES), c.id
    assert {c.id for c in st.EXTRA} == {"denv16-collect", "denv16-solve-actions", "denv16-evaluate", "policy-update-mfma", "policy-update-generic", "policy-evaluate"}
    # run d: every collect of a Puzzle or of a device environment, no evaluate / solve / hand-off / host-stepped case
    assert {c.family for c in st.CASES if st.MODE2 in c.modes} == set(st.MODE2_FAMILIES)


def test_census_of_the_users_of_the_library_stream():
    got = count_stream_users()
    want = {f: {fn: n for fn, (n, _) in fns.items()} for f, fns in st.STREAM_USERS.items()}
    assert got == want, (got, want)
    assert st.STREAM_COUNTS == {"tw_api.hip": 20, "tw_common.hpp": 1, "tw_device_env.hip": 7, "tw_env_generic.hip": 4, "tw_comm.hip": 1}
    assert st.STREAM_USERS["tw_comm.hip"] == {"tw_comm_broadcast_policy": (1, "multi-rank, not run here")}


def test_census_notices_a_new_user_of_the_stream(tmp_path):
    """A copy of the sources with one more `current_stream()` in a function the table knows, and one in a function it does not."""
    import shutil
    for name, old, new in (("tw_eval.hip", "namespace tw {", "namespace tw {\nint fresh_user() { return current_stream() != nullptr; }"),
                           ("tw_api.hip", "hipStream_t stream = nullptr;           // the library stream", "hipStream_t stream = current_stream();  // the library stream")):
        dst = tmp_path / name.replace(".", "_")
        shutil.copytree(CSRC, dst)
        text = (dst / name).read_text()
        assert old in text, (name, old)
        (dst / name).write_text(text.replace(old, new, 1))
        got = count_stream_users(str(dst))
        assert got != count_stream_users(), name
        assert sum(got[name].values()) == sum(count_stream_users().get(name, {}).values()) + 1


def test_every_entry_point_of_the_table_is_run_or_says_why_not():
    from twisterl_amd import _lib
    reached = {e for c in st.CASES for e in c.entries}
    assert reached <= set(st.LISTED) <= set(_lib.SYMBOLS), reached - set(st.LISTED)
    assert set(st.UNLISTED) <= set(_lib.SYMBOLS) and not set(st.UNLISTED) & set(st.LISTED)
    named = set()
    for f, fns in st.STREAM_USERS.items():
        for fn, (n, entries) in fns.items():
            if entries == st.NOT_RUN:
                assert (f, fn) == ("tw_comm.hip", "tw_comm_broadcast_policy")
                continue
            assert entries or fn == "current_stream", (f, fn)
            named |= set(entries)
    assert named <= set(_lib.SYMBOLS), named - set(_lib.SYMBOLS)
    # every entry point that reaches a user of the stream is delayed in some case, or is one of the four named exceptions
    assert named - reached == set(st.UNLISTED), (named - reached, set(st.UNLISTED))
    assert reached <= named, reached - named
    for c in st.CASES:
        assert c.entries and set(c.modes) <= {st.MODE1, st.MODE2}, c.id
    # what may never be exempt from run d: the Puzzle collectors
    for cid in st.MODE2_EXEMPT:
        assert st.MODE2 in st.BY_ID[cid].modes and not set(st.BY_ID[cid].entries) & {"tw_ppo_collect", "tw_az_collect"}, cid


def test_library_stream_is_bound_and_documented():
    from twisterl_amd import _lib
    assert "tw_set_stream" in _lib.SYMBOLS and "thread" in _lib.library_stream.__doc__.lower()
    for bad in ("stream", 1.5, -1):
        with pytest.raises(TypeError):
            _lib.library_stream(bad)

    class Fake:
        cuda_stream = 0
    assert _lib.library_stream(Fake()).handle == 0 and _lib.library_stream(None).handle == 0
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tests/test_gpu_stream_matrix.py" in text and "tests/test_gpu_threads.py" in text
    assert "tests/test_gpu_stream_matrix.py" in open(os.path.join(ROOT, "README.md")).read()
