"""The rule of a raw session's automatic query start (sfa_session_raw_auto_start) restated on the host, for the tests.

target(N) is the library's host twin api.auto_start_target on the slot's first N samples; the events are the host stream's
(api.EventStream).  Everything else -- the points, freezing, the skip, the fallback, the cap -- is restated here from the
samples a slot has received: feed() takes the chunks of a schedule, but every decision is a function of sample counts.
points_between() is the twin of auto_points (sigfish_amd/csrc/session_plan.hpp), the rule the library schedules a call's points
with; test_session_plan_cpu.py compares the two."""
import numpy as np

import sigfish_amd as S

FALLBACK = 50


def points_between(have, after, ended_now, every, max_samples):
    """the points a slot passes when its count of samples goes from `have` to `after`: ([periodic N_k, ascending], final N or None).
    A periodic point equal to the final point is the final point."""
    lo, hi = min(have, max_samples), min(after, max_samples)
    final = hi if (ended_now or (after >= max_samples and have < max_samples)) else None
    pts = [] if every <= 0 else [k * every for k in range(lo // every + 1, hi // every + 1)]
    return [p for p in pts if p != final], final


class AutoTwin:
    """what a slot of a session with the automatic start must hold after every call"""

    def __init__(self, meta, pore, every, max_samples, max_skip, query, rna=True):
        self.meta, self.pore, self.every, self.max_samples, self.max_skip, self.query, self.rna = meta, pore, every, max_samples, max_skip, query, rna
        self.reset()

    def reset(self):
        self.es = S.EventStream(self.meta, self.rna)
        self.ev = np.zeros(0, S.EVENT_DTYPE)
        self.kept = np.zeros(0, np.int16)
        self.n, self.ended, self.final_done = 0, False, False
        self.target, self.skip, self.frozen_at, self.status = -1, -1, 0, S.AUTO_PENDING
        self.targets = {}
        self.frozen_call = self.resolved_call = None
        self.table_full = False  # (of a BEYOND_MAX: the table was full below the target)
        self.calls = 0

    def final(self):
        return self.ev[:self.max_skip + self.query]

    def target_of(self, n):
        if n not in self.targets:
            self.targets[n] = S.auto_start_target(self.kept[:n], self.meta, self.pore)
        return self.targets[n]

    def feed(self, chunk, end):
        chunk = np.asarray(chunk, np.int16)
        self.calls += 1
        if not self.ended:
            self.ev = np.concatenate([self.ev, self.es.push(chunk)] + ([self.es.finish()] if end else []))
        have, after = self.n, self.n + len(chunk)
        ended_now = bool(end) and not self.ended
        self.n, self.ended = after, self.ended or bool(end)
        if len(self.kept) < self.max_samples:
            self.kept = np.concatenate([self.kept, chunk[:self.max_samples - len(self.kept)]])
        if self.target < 0 and not self.final_done:
            pts, final = points_between(have, after, ended_now, self.every, self.max_samples)
            for n in pts + ([final] if final is not None else []):
                t = self.target_of(n)
                if t >= 0:
                    self.target, self.frozen_at, self.frozen_call = t, n, self.calls
                    self.status = S.AUTO_PENDING | (S.AUTO_AT_FINAL if n == final else 0)
                    break
            if self.target < 0 and final is not None:
                self.frozen_at, self.skip, self.status = final, FALLBACK, S.AUTO_NO_TARGET | S.AUTO_AT_FINAL
                self.resolved_call = self.calls
            self.final_done = self.final_done or final is not None
        if self.skip < 0 and self.target >= 0:
            fin = self.final()
            idx = int(np.searchsorted(fin["start"], np.uint64(self.target), "left"))
            state = None
            if idx < len(fin) and idx <= self.max_skip:
                self.skip, state = idx, S.AUTO_RESOLVED
            elif idx < len(fin) or len(fin) >= self.max_skip + self.query:
                self.skip, state = FALLBACK, S.AUTO_BEYOND_MAX
                self.table_full = idx >= len(fin)
            elif self.ended:
                self.skip, state = FALLBACK, S.AUTO_NO_EVENT
            if state is not None:
                self.status = (self.status & ~15) | state
                self.resolved_call = self.calls

    def state(self):
        return (self.target, self.frozen_at, self.skip, self.status)

    def failed(self):
        return (self.status & 15) >= S.AUTO_NO_TARGET

    def q_avail(self):
        return 0 if self.skip < 0 else max(0, min(len(self.final()) - self.skip, self.query))


def cut(n, sizes):
    out, at, i = [], 0, 0
    while at < n:
        c = min(sizes[i % len(sizes)], n - at)
        out.append(c)
        at += c
        i += 1
    return out
