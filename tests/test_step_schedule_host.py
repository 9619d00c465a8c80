"""The stream schedule of as_artspeech_fwd / as_artspeech_bwd / as_artspeech_dw2 (csrc/artspeech.hip: Lanes, Fork, join) on the
host: what must hold for every schedule the step can take, read from the host-only call trace.

tools/head_stack_host_trace.cpp and a host-only compile of csrc/artspeech.hip are linked with lin_plan.cpp and run as a child
process (`--small`: one geometry, every mode and option set; nothing is preloaded, no GPU is opened: every HIP call is a stub
of the tool).  Each entry-point call of the output is replayed as a happens-before relation -- a launch is ordered behind the
launches before it on its stream; an event carries what its stream held when it was recorded, or when a launch carried it on
its own dispatch (mode 256); a wait hands that to the waiting stream -- and the invariants below are asserted on it.  They
hold for the schedule as it stood before Lanes / Fork existed as well (the trace of that code is equal as text:
profiles/step_schedule_equivalence.log).  What they do not see is which data a launch reads: a side stream that has waited
for one fork passes "fork before work" for everything behind it, so a dropped second fork is the GPU tests' to find."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "artspeech_amd", "csrc")
NOT_A_LAUNCH = ("#", "@", "prof<", "prof>", "slot=", "slot>", "hipEventRecord", "hipStreamWaitEvent", "as_set_error")
EXTERNAL = "Eext"   # as_opts.fold_wait_event: the caller's event, recorded outside the call
PLAIN, CAPTURING, CARRY, NO_DEVICE, FRESH_STREAM, L0_FAILS = 32, 128, 256, 64, 512, 1024


class Call:
    """One entry-point call: its header's fields, its lines, and the replay."""

    def __init__(self, header, what, v, caller):
        self.mode, self.simple = int(header["mode"]), int(header["simple"])
        self.where = " ".join(f"{k} {x}" for k, x in header.items()) + f" {what} v{v}"
        self.what, self.v, self.caller, self.lines = what, v, caller, []
        self.rc = self.slot = None

    def flat(self):
        """schedules with nothing beside the caller's stream: overlap off, no device, a capture on a stream without state,
        SimpleArtSpeech (no recurrence to work beside), the heads alone"""
        return (self.v == 3 or self.mode & (NO_DEVICE | FRESH_STREAM) or self.simple or self.what in ("head_fwd", "head_bwd", "dw2"))

    def replay(self):
        """-> problems found (strings).  know[s][t]: index of the last launch on stream t that stream s's next launch is
        ordered behind."""
        bad = []
        know, event, last, waited, slabs = {}, {}, {}, set(), {}
        armed, n_launch, prev = None, 0, None   # prev: (index, stream) of the launch the @ lines belong to
        self.records_on_caller = self.arms = 0
        self.launch_streams, self.waits, self.records = set(), [], []

        def behind(s):
            return know.setdefault(s, {})

        for line in self.lines:
            tok = line.split()
            if tok[0] == "hipEventRecord":
                e, s = tok[1], tok[2]
                event[e] = (s, dict(behind(s)))
                self.records.append((e, s))
                self.records_on_caller += s == self.caller
            elif tok[0] == "hipStreamWaitEvent":
                s, e = tok[1], tok[2]
                self.waits.append((s, e))
                if e == EXTERNAL:
                    waited.add(s)
                elif e not in event:
                    bad.append(f"wait on {s} for {e}, which nothing has recorded or carried in this call")
                elif event[e][0] == s:
                    bad.append(f"wait on {s} for {e}, recorded on the same stream")
                else:
                    waited.add(s)
                    for t, i in event[e][1].items():
                        behind(s)[t] = max(behind(s).get(t, -1), i)
            elif tok[0] == "slot=":
                armed = None if tok[1] == "E-" else tok[1]
                self.arms += armed is not None
            elif tok[0] == "slot>":
                armed = None
            elif tok[0] == "@carry":
                e, s = tok[1], tok[2]
                if e != armed or prev is None or prev[1] != s:
                    bad.append(f"{e} carried by a launch on {s} while the slot held {armed}")
                armed = None
                event[e] = (s, dict(behind(s)))
            elif tok[0] == "@slab":
                p, s = tok[1], tok[2]
                if p in slabs and slabs[p][1] != s and behind(s).get(slabs[p][1], -1) < slabs[p][0]:
                    bad.append(f"slab {p} used on {s} by launch {prev[0]}, unordered behind launch {slabs[p][0]} on {slabs[p][1]}")
                slabs[p] = prev
            elif not line.startswith(NOT_A_LAUNCH):
                streams = [t for t in tok[1:] if re.fullmatch(r"S(\d+|-)", t)]
                assert len(streams) == 1, line[:200]
                s = streams[0]
                if s != self.caller and s not in waited:
                    bad.append(f"{tok[0]} on {s} before that stream waited for anything")
                behind(s)[s] = n_launch
                last[s] = n_launch
                prev = (n_launch, s)
                self.launch_streams.add(s)
                n_launch += 1
        if self.rc == 0:
            for s, i in last.items():
                if s != self.caller and behind(self.caller).get(s, -1) < i:
                    bad.append(f"returns with launch {i} on {s} not joined to the caller's stream")
        return bad


@pytest.fixture(scope="module")
def calls(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("step_schedule")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = ["-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
    host_only = ["-x", "hip", "--offload-arch=gfx950", "--cuda-host-only"]   # (no kernel in either file)
    objs = []
    for src, opt, how in ((os.path.join(CSRC, "artspeech.hip"), "-O1", host_only), (os.path.join(CSRC, "lin_plan.cpp"), "-O1", []),
                          (os.path.join(ROOT, "tools", "head_stack_host_trace.cpp"), "-O1", host_only)):
        objs.append(str(tmp / (os.path.basename(src) + ".o")))
        subprocess.check_call([hipcc, opt, *inc, *how, "-c", src, "-o", objs[-1]])
    exe = str(tmp / "head_stack_host_trace")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", *objs, "-o", exe])
    run = subprocess.run([exe, "--small"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    out, header, cur = [], None, None
    for line in run.stdout.splitlines():
        if line.startswith("## "):
            f = line.split()
            header = dict(zip(f[1::2], f[2::2]))
        elif line.startswith("# call "):
            _, _, what, v, caller = line.split()
            cur = Call(header, what, int(v[1:]), caller)
        elif line.startswith("# "):
            _, what, v, rc, _, slot = line.split()
            assert cur is not None and (what, int(v[1:])) == (cur.what, cur.v), line
            cur.rc, cur.slot = int(rc), slot
            cur.problems = cur.replay()
            out.append(cur)
            cur = None
        else:
            assert cur is not None, line[:200]
            cur.lines.append(line)
    assert cur is None and len(out) >= 2000, len(out)   # 22 modes x 4 geometries x 23 calls
    return out


def test_trace_covers_the_schedules(calls):
    """every kind of schedule is in the trace: forks carried by a launch, forks recorded, side streams in use, flat calls, the
    deferred update's external event, and a backward that fails inside a fork's scope"""
    bwd = [c for c in calls if c.what == "bwd" and not c.flat()]
    assert any(c.arms and "@carry" in "\n".join(c.lines) for c in bwd if c.mode & CARRY)
    assert any(c.arms and "@carry" not in "\n".join(c.lines) for c in bwd if not c.mode & CARRY)
    assert any(len(c.launch_streams) == 3 for c in bwd)
    assert any((s, EXTERNAL) in c.waits for c in calls if c.what == "fwd" and c.v == 4 for s in c.launch_streams)
    assert any(c.flat() for c in calls if c.what == "bwd" and c.mode & FRESH_STREAM)
    assert any(c.rc != 0 and c.arms for c in calls if c.mode & L0_FAILS)
    assert all(c.rc == 0 for c in calls if not c.mode & L0_FAILS)


def test_side_work_is_forked_ordered_and_joined(calls):
    """Fork before work: a launch on a stream other than the caller's comes behind a wait of that stream.  Every wait has a
    producer: an earlier record, on another stream, or an armed event that a launch carried (the external fold_wait_event
    aside).  Everything is joined: at a successful return the caller's stream is ordered behind the last launch of every other
    stream.  Slabs are not shared unordered: a slab used on two streams is used by the second behind the first's launch."""
    found = [f"{c.where}: {p}" for c in calls for p in c.problems]
    assert not found, "\n".join(found[:20])


def test_the_slot_never_leaks(calls):
    """at every return, an error return included, the stop-event slot is empty: no later launch of the thread binds a fork's
    event to its own completion"""
    leaks = [f"{c.where}: returned {c.rc} with {c.slot} armed" for c in calls if c.slot != "E-"]
    assert not leaks, "\n".join(leaks[:20])


def test_degenerate_schedules_are_flat(calls):
    """overlap off, no device, a capture on a stream the library has no state for (and the calls that have no side work): every
    launch on the caller's stream, no fork, no join -- the only event calls are the "head gradients are final" record on the
    caller's stream and, on it as well, the wait for the external fold_wait_event"""
    flat = [c for c in calls if c.flat()]
    assert flat
    for c in flat:
        assert c.launch_streams <= {c.caller}, c.where
        assert all(s == c.caller for _, s in c.records) and c.arms == 0, c.where
        assert all(w == (c.caller, EXTERNAL) for w in c.waits), c.where
    # and a call that is not flat does use a side stream (the forward's folds, the backward's weight gradients)
    assert all(len(c.launch_streams) >= 2 for c in calls if not c.flat()), [c.where for c in calls if not c.flat() and len(c.launch_streams) < 2][:5]


def test_forks_ride_or_are_plain_records(calls):
    """With the timers on (mode 32) or inside a capture (mode 128) nothing is armed: every fork is a record.  Otherwise, when
    the launchers take an armed event (mode 256), the backward's critical stream sees no record at all -- except the one behind
    the inter-layer dropout, which follows the GEMM the fork would have ridden on (option sets 1 and 3: dropout on)."""
    for c in calls:
        if c.what != "bwd" or c.flat() or c.rc != 0:
            continue
        if c.mode & (PLAIN | CAPTURING):
            assert c.arms == 0 and c.records_on_caller == 3, c.where
        elif c.mode & CARRY:
            assert c.records_on_caller == (1 if c.v & 1 else 0), c.where
