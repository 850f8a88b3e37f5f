"""The replay of `sigfish-amd realtime` in Python: reads go through a raw-signal Session as a flow cell would deliver them.

Twin of sigfish_amd/csrc/cli/replay.hpp (the schedule and the decision rule) and cli/realtime_main.cpp (the run): the same
ticks, the same calls, the same lines.  The schedule counts ticks, never seconds.

  setup     read i goes to channel i, i < channels
  tick t    every busy channel sends the next chunk_samples samples of its read, ascending channels, in ONE extend_raw call; a
            chunk shorter than chunk_samples (empty when the read's length is a multiple of it) is the last and carries the end
  windows   with recalibrate / at_end the session renormalises a slot over a longer window as it grows (api.recal_window) and sweeps
            it again inside the call; the schedule and the decision rule do not change
  resweep   --resweep: the session is created with SESSION_RESWEEP (a slot is swept only when its window changes, over the
            window's events; what direct RNA without --invert needs); schedule and rule are the same, q_events counts the window
  decision  decide(): 'E' early (calibrated, q_events >= min_events, mapped, mapq >= min_mapq), 'F' full, 'R' end of read (or a
            poisoned slot); a decision has a line when its row is mapped
  candidates --candidates N: the session keeps N candidates per slot (Session.configure_candidates); those of all channels
            decided in a tick are fetched in one Session.candidates call before the reset, and a channel's valid ones follow its
            primary line, best first (format_candidates)
  auto start skip = -1 (-p -1, with resweep on an RNA aligner without INV): the session finds each read's query start behind the
            adaptor and the poly-A tail as it streams (Session.configure_auto_start: a point every auto_start_every samples, the
            final point at the end of the read or at auto_start_max_samples); max_skip_events is the largest skip.  Schedule and
            rule are unchanged: a channel with no skip yet is simply not calibrated.  A decision carries the channel's automatic
            start, and its line two more tags, qs:i:<skip> as:A:<P|E|F> (found at a mid-read point, at the final point, fallback)
  sam       sam=True (Python only; the binary refuses --sam): a decided channel prints the SAM record of its row instead of the PAF
            line.  The maps of all rows decided in a tick -- primaries, and candidates under candidates=N -- come from ONE
            Session.event_maps call before the reset, on the slots' resident queries; the record is sam_row_from_map over the slot's
            events (Session.events) and is followed by the same tags (format_sam_line, format_sam).  Schedule and rule are unchanged
  spread    --spread: the session is created with SESSION_SPREAD on an Aligner over several devices; nothing else changes
  targets   targets= (--targets FILE.bed with --enrich or --deplete and --margin X): the session gets the intervals
            (Session.set_targets), every tick ends with ONE Session.classes call over the tick's channels, and the 'E' test of
            decide() is replaced by api.target_decide on the channel's class record (decide_targets); 'F' and 'R' stay.  Every line
            gains tc:A:<T|O|N> ac:A:<A|U|P> tm:f:<(other - mine) / n_events> (target_tags).  An accepted ('A') or proceeding ('P')
            read keeps its channel for ceil((len - sent) / chunk) further ticks without sending (trace: `hold ... left=K`); an
            unblocked one frees it at once.  Refused with resweep (the session refuses targets there).  margin has no default
  quota     quota=N with by_name=True and mode=ENRICH (--quota N): every named group wants N accepted reads.  The tick's
            Session.classes call is replaced by ONE Session.open_classes call under the bitmap of the groups still open when the tick
            began; decisions run on its `cls` unchanged.  Every read accepted ('A') with a line is credited to its on_group in
            ascending channel order (api.QuotaBook, in Schedule.end_tick); the credit that fills a quota closes the group from the
            next tick on (trace: `close group=NAME accepted=K`), so a group may overshoot by the reads accepted in its closing
            tick.  Proceeding reads are not credited.  Lines gain og:Z:<name of on_group, * for none> (quota_tags)
  depth cap depth_cap=N with mask targets and mode=ENRICH (--depth-cap N; not with by_name / quota): the session keeps a depth track
            (Session.configure_coverage).  At the end of a tick the reads accepted in it ('A', with a line) add the target interval of
            their line, [pos_st, pos_end) of the row's contig, in ONE Session.add_coverage call, ascending channels; the live mask
            it derives holds from the next tick on (trace: `tick T cover n=K open=M`).  summary["cover"]: format_cover_summary
  truth     truth= (--truth FILE.paf; needs targets=): {read id: (contig, begin, end)} as api.read_truth returns it.  Every decided read
            is looked up once, at its decision: its true class (api.truth_class: 'T' when its interval shares a base with a target,
            'O' when not or when it belongs nowhere, 'N' when it has no truth) and the verdict of the decided class
            (api.truth_verdict: 'C', 'W', 'N'); with by_name the true group and the verdict of the line's tg.  Lines gain tt:A / tv:A
            (tn:Z / gv:A) behind all other tags (truth_tags), the trace one `verdict ch=C read=R tt=X tv=Y sent=S` line behind every
            `decide` line, summary["truth"] the account (format_truth_summary).  Truth changes no decision
  after it  decided channels are reset in one call and take the next unread reads, lowest channel first, from tick t + 1 on
"""
import numpy as np

from . import api


def mapped(row):
    return bool(row["valid"]) and int(row["rid"]) >= 0


def decide(row, info, min_events, min_mapq):
    """'E', 'F', 'R' or None for one channel after a call (replay::decide)."""
    st = int(info["status"])
    if st & api.RAW_CALIBRATED and int(info["q_events"]) >= min_events and mapped(row) and int(row["mapq"]) >= min_mapq:
        return "E"
    if st & api.RAW_FULL:
        return "F"
    if st & (api.RAW_ENDED | api.RAW_POISONED):
        return "R"
    return None


def decide_targets(info, decision):
    """replay::decide_targets: `decision` is api.target_decide of the channel's class record ('A', 'U' or None)"""
    st = int(info["status"])
    if st & api.RAW_CALIBRATED and decision:
        return "E"
    if st & api.RAW_FULL:
        return "F"
    if st & (api.RAW_ENDED | api.RAW_POISONED):
        return "R"
    return None


def action_of(reason, decision):
    """what happens to a decided read: the class decision when it was early, else it proceeds ('P')"""
    return decision if reason == "E" else "P"


class Schedule:
    """replay::Schedule: which read is on which channel and which samples go out at which tick.  `source.take(channel)` puts the
    next unread record of the file on the channel and returns its length (None: the file has no more); `trace`, a list, receives
    the lines the C++ schedule prints."""

    def __init__(self, channels, chunk_samples, trace=None, resweep=False, targets=False):
        self.chunk, self.trace = int(chunk_samples), trace
        self.targets, self.hold = bool(targets), [0] * channels  # hold: ticks a channel still keeps a decided read without sending
        self.resweep = bool(resweep)  # of the session; nothing here reads it: the schedule does not depend on it
        self.read, self.len, self.sent = [-1] * channels, [0] * channels, [0] * channels
        self.tick, self.next_read, self.entries = 0, 0, []
        self.book = self.names = None  # set_quota
        self.closed_at = []

    def set_quota(self, book, names):
        """replay::Schedule::set_quota: the api.QuotaBook accepted reads are credited in, and the groups' names"""
        self.book, self.names, self.closed_at = book, names, [-1] * book.n_groups

    def _take(self, c, source):
        n = source.take(c)
        if n is None:
            return False
        self.read[c], self.len[c], self.sent[c] = self.next_read, int(n), 0
        self.next_read += 1
        if self.trace is not None:
            self.trace.append(f"tick {self.tick} take ch={c} read={self.read[c]} len={self.len[c]}")
        return True

    def start(self, source):
        for c in range(len(self.read)):
            if not self._take(c, source):
                break

    def busy(self):
        return any(r >= 0 for r in self.read)

    def begin_tick(self):
        """[(channel, read, first, count, end)], ascending channels; the samples count as sent"""
        self.entries = []
        for c, r in enumerate(self.read):
            if r < 0:
                continue
            if self.hold[c] > 0:  # (only with targets)
                if self.trace is not None:
                    self.trace.append(f"tick {self.tick} hold ch={c} read={r} left={self.hold[c]}")
                continue
            n = min(self.chunk, self.len[c] - self.sent[c])
            self.entries.append((c, r, self.sent[c], n, n < self.chunk))
            self.sent[c] += n
            if self.trace is not None:
                self.trace.append(f"tick {self.tick} send ch={c} read={r} first={self.entries[-1][2]} n={n} end={int(n < self.chunk)}")
        return self.entries

    def end_tick(self, reason, line, source, action=None, on_group=None, truth=None):
        """action (with targets): action_of per entry; on_group (with a quota): the open-class record's per entry; truth (with
        truth): (tt, tv) per entry, None for an undecided one; -> samples every entry's read is held for (0 without targets)"""
        if self.targets and action is not None:
            return self._end_tick_targets(reason, line, source, action, on_group, truth)
        for (c, r, _, _, _), why, ln in zip(self.entries, reason, line):
            if not why:
                continue
            if self.trace is not None:
                self.trace.append(f"tick {self.tick} decide ch={c} read={r} reason={why} line={int(bool(ln))} sent={self.sent[c]}")
            self.read[c] = -1
        for (c, _, _, _, _), why in zip(self.entries, reason):
            if why and not self._take(c, source):
                break
        self.tick += 1
        return [0] * len(self.entries)

    def _end_tick_targets(self, reason, line, source, action, on_group=None, truth=None):
        held = [0] * len(self.entries)
        freed = [False] * len(self.read)
        for c in range(len(self.read)):  # holds of earlier ticks: one tick less, the last one frees
            if self.read[c] >= 0 and self.hold[c] > 0:
                self.hold[c] -= 1
                freed[c] = self.hold[c] == 0
        for i, ((c, r, _, _, _), why, ln) in enumerate(zip(self.entries, reason, line)):
            if not why:
                continue
            if self.trace is not None:
                self.trace.append(f"tick {self.tick} decide ch={c} read={r} reason={why} line={int(bool(ln))} sent={self.sent[c]}")
                if truth is not None:
                    self.trace.append(f"tick {self.tick} verdict ch={c} read={r} tt={truth[i][0]} tv={truth[i][1]} sent={self.sent[c]}")
            if self.book is not None and on_group is not None and action[i] == "A" and ln and self.book.note_accept(int(on_group[i])):
                g = int(on_group[i])  # this read filled its group's quota
                self.closed_at[g] = self.tick
                if self.trace is not None:
                    self.trace.append(f"tick {self.tick} close group={self.names[g]} accepted={self.book.accepted[g]}")
            ticks = 0 if action[i] == "U" else -(-(self.len[c] - self.sent[c]) // self.chunk)
            if ticks > 0:
                self.hold[c], held[i] = ticks, self.len[c] - self.sent[c]
            else:
                freed[c] = True
        more = True
        for c in range(len(self.read)):
            if freed[c]:
                self.read[c], self.hold[c] = -1, 0
                if more:
                    more = self._take(c, source)
        self.tick += 1
        return held


def recal_points(norm, query, recalibrate=(), at_end=False):
    """The points `sigfish-amd realtime` hands its session: the list (or api.recal_double for "double"); with at_end the query size
    joins them unless it is the last already, so that a read that ends FULL is normalised over the query as one that ends short is
    over all it has (the session's RECAL_AT_END)."""
    at = tuple(api.recal_double(norm, query) if isinstance(recalibrate, str) and recalibrate == "double" else recalibrate)
    if at_end and query > norm and (not at or at[-1] != query):
        at += (query,)
    return at


AUTO_START_MAX_SAMPLES, MAX_SKIP_EVENTS = 131072, 4096  # the defaults of --auto-start-max-samples and --max-skip-events


def replay(aligner, reads, channels, chunk_samples, skip, norm, query, min_events, min_mapq, session=None, trace=None, recalibrate=(), at_end=False, resweep=False,
           candidates=0, auto_start_every=None, auto_start_max_samples=AUTO_START_MAX_SAMPLES, max_skip_events=MAX_SKIP_EVENTS, sam=False, spread=False, targets=None, mode=None, margin=None, summary=None, by_name=False, quota=None, truth=None, depth_cap=None, group_cap=None, lead=None, stranded=False,
           group_lead=None, group_stranded=False):
    """Generator of (tick, channel, read_index, row, info, span, reason), one per decided read, in tick then channel order.
    candidates=1..4 (--candidates): an eighth element, RESULT_DTYPE[4], the channel's candidates at the decision, best first.
    A `session` of the caller's is taken as it is, in this as in its raw mode: it must keep that many candidates already
    (Session.configure_candidates), which is checked before the first tick.

    reads: iterable of (read_id, meta, samples) in file order, as Blow5File yields them (taken lazily: at most `channels` reads are
    held).  row / info: the channel's entries of Session.extend_raw at the decision; span: (start_raw, end_raw) of
    Session.query_span; reason: 'E', 'F' or 'R'.  A decision has a line when mapped(row): format_line().  `session`: an object with
    extend_raw / query_span / reset in place of aligner.session(channels) in raw mode (the schedule's tests pass a stub).
    recalibrate / at_end: --recalibrate (a list of window lengths, or "double": api.recal_double(norm, query)) and
    --recalibrate-at-end, turned into the session's points by recal_points(); schedule and decision rule are the same with them.
    resweep: --resweep, the session is aligner.session(channels, resweep=True); info["q_events"], which the rule and the line read,
    is then the slot's window.
    skip = -1 (-p -1): the automatic query start; needs resweep.  auto_start_every (None: chunk_samples; 0: the final point only),
    auto_start_max_samples and max_skip_events configure it on a session of replay's own; every item then ends with one more
    element, the channel's SESSION_AUTO_DTYPE record at the decision, which format_line takes as auto=.
    sam=True: every item ends with one element more, behind all others, what format_sam() needs for the decision's SAM records: a
    dict with `events` (Session.events of the slot), `qstart` / `qend` (the query inside them: the slot's skip and skip + q_events),
    `map` (the primary's int32 [n, 2] event map from Session.event_maps, None when it has none) and `cand_maps` (the four
    candidates' maps with candidates=N, else None).  A session that carries no start columns (starts=False) has no maps: refused
    before any call.
    spread=True (--spread): the session of replay's own is aligner.session(channels, spread=True) -- on an Aligner made with
    devices= the channels are dealt over its devices; the items are the same.
    by_name=True (--by-name): targets= is the pair api.read_target_groups returns, (GROUP_TARGET_DTYPE array, group names): its
    intervals are the targets, and its groups become the session's (Session.set_target_groups).  Decisions stay the class
    record's; every tick ends with ONE Session.group_bests call over the channels that have a line in it, and an item gains, behind
    the class record and the action, the channel's GROUP_HEAD_DTYPE record (None without a line), which format_line takes as
    group=(head, names).  summary gains ("group", index) -> accepted reads whose best entry that is.
    quota=N (--quota N; needs by_name=True and mode=ENRICH, N >= 1): see `quota` above.  An item's class record is the open-class
    record's `cls`, and the item gains, behind the head, the record's on_group (format_line takes quota=(on_group, names)).
    summary gains "quota" -> N and ("closed_at", index) -> the tick whose credit closed the group.
    truth={read id: (contig, begin, end)} (--truth FILE.paf; api.read_truth; needs targets=): see `truth` above.  An item gains, behind
    the on_group (or whatever came last of the class record, the head and it), a dict with tt, tv and edge, and with by_name
    true_group (None: the read has no truth) and gv (None: the read has no line) -- format_line takes it as truth=(that dict, names).
    summary gains "truth", the account format_truth_summary prints.
    depth_cap=N (--depth-cap N; needs mask targets= with mode=ENRICH, N >= 1, a session that carries start columns): see `depth
    cap` above.  The items are unchanged; summary gains "cover", a dict with cap, intervals, bases, open and base (columns).
    group_cap=N (--group-cap N; needs by_name=True and mode=ENRICH, N >= 1, a session that carries start columns; quota= is
    optional with it; not with depth_cap, mode=DEPLETE or resweep): the session keeps a depth track and a live label table
    (Session.configure_group_coverage).  One Session.open_classes call per tick decides -- under the quota book's bitmap, or every
    group open without a quota -- and the items gain the on_group as with a quota.  At the end of a tick the accepted reads'
    [pos_st, pos_end) go into ONE Session.add_coverage call, ascending channels (trace: `tick T cover n=K open=M`); the live table
    holds from the next tick on.  Then one Session.group_coverage call: a group whose every column is capped for the first time
    is reported as `tick T full group=NAME`.  summary gains "group_cover": cap, intervals, bases and records (format_group_cover_summary).
    lead=N (--lead N; needs mask targets=, 0 <= N <= 2^30; not with by_name / quota / group_cap, allowed with depth_cap and truth): the
    session's targets are reach targets (Session.set_reach_targets) -- every interval with the lead N in front of it in the read's
    direction.  stranded=True (--stranded; needs lead=): targets= is a REACH_TARGET_DTYPE array whose strands are kept
    (api.read_reach_targets(path, names, N, stranded=True)); without it every target is for both strands.  Schedule, decision
    rule, items and tags are unchanged; truth reads the intervals without their leads.  summary gains "reach": lead, stranded
    and columns, the on-target columns (format_reach_summary).
    group_lead=N (--group-lead N; needs by_name=True and mode=ENRICH, 0 <= N <= 2^30; quota, group_cap and truth are optional with it;
    not with lead, depth_cap or mode=DEPLETE): the session's label table is a reach label table
    (Session.set_reach_target_groups) -- the N bases in front of every named target, in the read's direction, carry the label of
    the target the read reaches first -- and its mask the reach mask of the same list with the same lead.  group_stranded=True
    (--group-stranded; needs group_lead=): targets= is the pair api.read_reach_target_groups(path, names, N, stranded=True)
    returns, whose strands are kept; without it every target is for both strands.  Items, tags, trace and the quota / cap
    behaviour are by_name's, over the reach labels; under group_cap a lead-in closes when the base it leads to is covered.  summary
    gains "reach_groups": lead, stranded and columns, the labelled columns (format_reach_group_summary)."""
    auto = skip < 0
    if group_lead is not None or group_stranded:  # (before any session exists, each with the fix)
        if not by_name:
            raise api.SfaError("replay: group_lead / group_stranded widen named groups in the read's direction: pass targets=(group targets, names), by_name=True, "
                               "mode=ENRICH and margin= with them")
        if lead is not None or stranded:
            raise api.SfaError("replay: group_lead and lead are two leads: with by_name pass group_lead alone (the mask gets the same lead)")
        if depth_cap is not None:
            raise api.SfaError("replay: group_lead with depth_cap is not built: depth_cap is for mask targets; the cap of named groups is group_cap")
        if mode == api.DEPLETE:
            raise api.SfaError("replay: group_lead with mode=DEPLETE is not built: use mode=ENRICH")
        if group_lead is None:
            raise api.SfaError("replay: group_stranded belongs to group_lead=: pass group_lead=N (0 for no lead-in) with it")
        if isinstance(group_lead, bool) or not isinstance(group_lead, (int, np.integer)) or group_lead < 0 or group_lead > api.REACH_LEAD_MAX:
            raise api.SfaError("replay: group_lead should be an integer 0..1073741824")
        if group_stranded and not (isinstance(targets, (tuple, list)) and len(targets) == 2 and isinstance(targets[0], np.ndarray) and targets[0].dtype == api.REACH_GROUP_TARGET_DTYPE):
            raise api.SfaError("replay: group_stranded=True takes targets= as the pair api.read_reach_target_groups(path, names, group_lead, stranded=True) returns")
    if lead is not None or stranded:  # (before any session exists, each with the fix)
        if targets is None:
            raise api.SfaError("replay: lead / stranded widen targets in the read's direction: pass targets= with mode= and margin= with them")
        if by_name or quota is not None or group_cap is not None:
            raise api.SfaError("replay: lead / stranded are for mask targets: with by_name / quota / group_cap they are not built (groups work from labels)")
        if lead is None:
            raise api.SfaError("replay: stranded belongs to lead=: pass lead=N (0 for no lead-in) with it")
        if isinstance(lead, bool) or not isinstance(lead, (int, np.integer)) or lead < 0 or lead > api.REACH_LEAD_MAX:
            raise api.SfaError("replay: lead should be an integer 0..1073741824")
        if stranded and not (isinstance(targets, np.ndarray) and targets.dtype == api.REACH_TARGET_DTYPE):
            raise api.SfaError("replay: stranded=True takes targets= as a REACH_TARGET_DTYPE array (api.read_reach_targets(path, names, lead, stranded=True))")
    if group_cap is not None:  # (before any session exists, each with the fix)
        if isinstance(group_cap, bool) or not isinstance(group_cap, (int, np.integer)) or group_cap < 1 or group_cap > 1 << 30:
            raise api.SfaError("replay: group_cap should be an integer 1..1073741824 (None for no cap)")
        if mode == api.DEPLETE:
            raise api.SfaError("replay: group_cap with mode=DEPLETE is not built: a covered position would turn on target; use mode=ENRICH")
        if not by_name or targets is None or mode != api.ENRICH:
            raise api.SfaError("replay: group_cap closes the covered columns of named groups: pass targets=(group targets, names), by_name=True, mode=ENRICH and margin= with it")
        if depth_cap is not None:
            raise api.SfaError("replay: group_cap and depth_cap are two caps over one depth track: pass one of them (depth_cap is for mask targets)")
        if resweep:
            raise api.SfaError("replay: group_cap is not available with resweep=True: a resweep session has no target groups")
        if session is not None and not getattr(session, "starts", True):
            raise api.SfaError("replay: group_cap needs the rows' start columns for the interval; the session was created with starts=False (SESSION_NO_START)")
    if depth_cap is not None:  # (before any session exists, each with the fix)
        if isinstance(depth_cap, bool) or not isinstance(depth_cap, (int, np.integer)) or depth_cap < 1 or depth_cap > 1 << 30:
            raise api.SfaError("replay: depth_cap should be an integer 1..1073741824 (None for no cap)")
        if mode == api.DEPLETE:
            raise api.SfaError("replay: depth_cap with mode=DEPLETE is not built: a covered position would turn on target; use mode=ENRICH")
        if targets is None or mode != api.ENRICH:
            raise api.SfaError("replay: depth_cap closes covered target positions: pass targets=, mode=ENRICH and margin= with it")
        if by_name or quota is not None:
            raise api.SfaError("replay: depth_cap is for mask targets: with by_name / quota it is not built (per-group base quotas)")
        if session is not None and not getattr(session, "starts", True):
            raise api.SfaError("replay: depth_cap needs the rows' start columns for the interval; the session was created with starts=False (SESSION_NO_START)")
    if truth is not None and targets is None:  # (before any session exists)
        raise api.SfaError("replay: truth= checks target decisions: pass targets= with mode= and margin= with it")
    if quota is not None:  # (before any session exists, each with the fix)
        if not by_name:
            raise api.SfaError("replay: quota counts accepted reads per named group: pass targets=(group targets, names), by_name=True and mode=ENRICH with it")
        if mode == api.DEPLETE:
            raise api.SfaError("replay: quota is not available with mode=DEPLETE (a closed group's reads would be accepted): use mode=ENRICH")
        if isinstance(quota, bool) or not isinstance(quota, (int, np.integer)) or quota < 1:
            raise api.SfaError("replay: quota should be an integer >= 1 (None for no quota)")
    if by_name and targets is None:
        raise api.SfaError("replay: by_name belongs to targets=")
    group_targets = group_names = None
    if by_name:
        group_targets, group_names = targets
        reach_groups = None
        if isinstance(group_targets, np.ndarray) and group_targets.dtype == api.REACH_GROUP_TARGET_DTYPE:  # (the strands are read only with group_stranded)
            reach_groups = group_targets
            group_targets = np.zeros(len(reach_groups), api.GROUP_TARGET_DTYPE)
            for f in ("contig", "begin", "end", "group"):
                group_targets[f] = reach_groups[f]
        group_targets = api._group_targets(group_targets)
        if group_lead is not None:  # the two reach lists for the session; `targets` and `group_targets` stay the plain intervals (truth reads them)
            reach_group_targets = np.zeros(len(group_targets), api.REACH_GROUP_TARGET_DTYPE)
            for f in ("contig", "begin", "end", "group"):
                reach_group_targets[f] = group_targets[f]
            reach_group_targets["lead"] = int(group_lead)
            if group_stranded:
                reach_group_targets["strand"] = reach_groups["strand"]
        targets = np.zeros(len(group_targets), api.TARGET_DTYPE)
        for f in ("contig", "begin", "end"):
            targets[f] = group_targets[f]
    reach_targets = None
    if lead is not None:  # the reach list for the session; `targets` stays the plain intervals (truth reads them)
        src_t = targets if isinstance(targets, np.ndarray) and targets.dtype == api.REACH_TARGET_DTYPE else api._targets(targets)
        reach_targets = np.zeros(len(src_t), api.REACH_TARGET_DTYPE)
        targets = np.zeros(len(src_t), api.TARGET_DTYPE)
        for f in ("contig", "begin", "end"):
            reach_targets[f] = targets[f] = src_t[f]
        reach_targets["lead"] = int(lead)
        if stranded:
            reach_targets["strand"] = src_t["strand"]
    if targets is None and (mode is not None or margin is not None):
        raise api.SfaError("replay: mode and margin belong to targets=")
    if targets is not None:  # (all of it before any session exists)
        if mode not in (api.ENRICH, api.DEPLETE):
            raise api.SfaError("replay: targets= needs mode=ENRICH or mode=DEPLETE")
        if margin is None:
            raise api.SfaError("replay: targets= needs margin=: nobody has measured a good value, there is no default")
        if resweep:
            raise api.SfaError("replay: targets= is not available with resweep=True: a resweep session's carried row belongs to the reversed query")
    if sam and session is not None and not getattr(session, "starts", True):
        raise api.SfaError("replay: sam=True needs the rows' start columns; the session was created with starts=False (SESSION_NO_START)")
    if auto and not resweep:
        raise api.SfaError("replay: skip = -1 (automatic query start) needs resweep=True on an RNA aligner without INV")
    reads = iter(reads)
    on = [None] * channels  # (index, read_id, meta, samples) per channel

    class Source:
        index = 0

        def take(self, channel):
            nxt = next(reads, None)
            if nxt is None:
                return None
            raw = np.ascontiguousarray(nxt[2], np.int16).reshape(-1)
            on[channel] = (self.index, nxt[0], nxt[1], raw)
            self.index += 1
            return len(raw)

    src = Source()
    sch = Schedule(channels, chunk_samples, trace, resweep, targets is not None)
    book = None
    if quota is not None and by_name:
        book = api.QuotaBook(len(group_names), int(quota))
        sch.set_quota(book, group_names)
        if summary is not None:
            summary["quota"] = int(quota)
    account = None
    if truth is not None:
        account = new_truth_account(by_name)
        if summary is not None:
            summary["truth"] = account
    own = session is None
    se = aligner.session(channels, resweep=resweep, spread=spread) if own else session
    try:
        if own:
            if candidates:
                se.configure_candidates(candidates)
            se.configure_raw(max_skip_events if auto else skip, norm, query, recal_points(norm, query, recalibrate, at_end), at_end)
            if auto:
                se.configure_auto_start(chunk_samples if auto_start_every is None else auto_start_every, auto_start_max_samples)
        if reach_targets is not None:
            se.set_reach_targets(reach_targets)
            if summary is not None:
                summary["reach"] = dict(lead=int(lead), stranded=bool(stranded), columns=se.target_columns())
        elif targets is not None and group_lead is None:
            se.set_targets(targets)
        if by_name and group_lead is not None:
            reach_mask = np.zeros(len(reach_group_targets), api.REACH_TARGET_DTYPE)
            for f in ("contig", "begin", "end", "lead", "strand"):
                reach_mask[f] = reach_group_targets[f]
            se.set_reach_targets(reach_mask)  # (in place of the plain mask: the same columns the labels name)
            se.set_reach_target_groups(reach_group_targets, len(group_names))
            if summary is not None:
                summary["reach_groups"] = dict(lead=int(group_lead), stranded=bool(group_stranded), columns=se.target_columns())
        elif by_name:
            se.set_target_groups(group_targets, len(group_names))
        cover = None
        if depth_cap is not None:
            cover = dict(cap=int(depth_cap), intervals=0, bases=0, base=se.target_columns())
            se.configure_coverage(depth_cap)
            cover["open"] = se.target_columns()
            if summary is not None:
                summary["cover"] = cover
        gcover = None
        if group_cap is not None:
            se.configure_group_coverage(group_cap)
            gcover = dict(cap=int(group_cap), intervals=0, bases=0, records=se.group_coverage(), full=set())
            if summary is not None:
                summary["group_cover"] = gcover
        use_open = book is not None or gcover is not None  # the tick's class call is open_classes; the items gain on_group
        if candidates and not own:
            se.candidates([])  # (raises unless the caller's session keeps candidates)
        sch.start(src)
        while sch.busy():
            es = sch.begin_tick()
            slots = [e[0] for e in es]
            chunks = [on[c][3][first:first + n] for c, _, first, n, _ in es]
            raw_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
            scaling = [(on[c][2]["digitisation"], on[c][2]["offset"], on[c][2]["range"]) for c in slots]
            sch_sent = [first + n for _, _, first, n, _ in es]  # samples of every entry's read sent so far
            rows, info = se.extend_raw(slots, np.concatenate(chunks) if chunks else np.zeros(0, np.int16), raw_off, scaling, [e[4] for e in es])
            cls = action = on_group = None
            if targets is not None:  # one call for the tick, before any reset
                if use_open:  # under the groups open at the start of the tick (the book changes in end_tick only; no book: every group)
                    ocls = se.open_classes(slots, None if book is None else book.open)
                    cls, on_group = ocls["cls"].copy(), ocls["on_group"].copy()
                else:
                    cls = se.classes(slots)
                dec = [api.target_decide(cls[i], mode, min_events, margin) for i in range(len(es))]
                reason = [decide_targets(info[i], dec[i]) for i in range(len(es))]
                action = [action_of(why, dec[i]) if why else None for i, why in enumerate(reason)]
            else:
                reason = [decide(rows[i], info[i], min_events, min_mapq) for i in range(len(es))]
            line = [bool(why) and mapped(rows[i]) for i, why in enumerate(reason)]
            decided = [i for i, why in enumerate(reason) if why]
            marks = None
            if truth is not None:  # one look-up per read, at its decision
                marks = [None] * len(es)
                for i in decided:
                    where = truth.get(on[slots[i]][1])
                    tt = "N" if where is None else api.truth_class(targets, *where)
                    marks[i] = dict(tt=tt, tv=api.truth_verdict(class_of_decision(dec[i], mode), tt), edge=where is not None and api.truth_edge(targets, *where), length=sch.len[slots[i]])
                    if by_name:
                        marks[i]["true_group"] = None if where is None else api.truth_group(group_targets, len(group_names), *where)
                        marks[i]["gv"] = None
            if decided:
                d_slots = [slots[i] for i in decided]
                a, b = se.query_span(d_slots)
                cand = se.candidates(d_slots) if candidates else None
                au = se.auto_start(d_slots) if auto else None
                maps = None
                if sam:  # one call for the tick: every decided channel's primary, then its four candidate rows
                    per = 5 if candidates else 1
                    m_rows = np.zeros(per * len(decided), api.RESULT_DTYPE)
                    for k, i in enumerate(decided):
                        m_rows[per * k] = rows[i]
                        if candidates:
                            m_rows[per * k + 1:per * k + 5] = cand[k]
                    pairs, off, _ = se.event_maps(m_rows, np.repeat(np.asarray(d_slots, np.int32), per))
                    maps = [_map_or_none(pairs[off[j]:off[j + 1]]) for j in range(len(m_rows))]
                heads = {}
                if by_name:  # one call for the tick, over the channels that have a line, before the reset
                    lined = [i for i in decided if line[i]]
                    if lined:
                        heads = dict(zip(lined, se.group_bests([slots[i] for i in lined])[1]))
                    if marks is not None:  # the line's tg names the head's best entry, the background for none
                        for i in lined:
                            best = int(heads[i]["best"])
                            marks[i]["gv"] = api.truth_group_verdict(best if 0 <= best < len(group_names) else len(group_names), marks[i]["true_group"])
                            account["groups"][marks[i]["gv"]] += 1
                    if summary is not None:
                        for i in lined:
                            if action[i] == "A" and heads[i]["best"] >= 0:
                                summary[("group", int(heads[i]["best"]))] = summary.get(("group", int(heads[i]["best"])), 0) + 1
                for k, i in enumerate(decided):
                    item = (sch.tick, slots[i], on[slots[i]][0], rows[i].copy(), info[i].copy(), (int(a[k]), int(b[k])), reason[i])
                    if candidates:
                        item += (cand[k].copy(),)
                    if targets is not None:
                        item += (cls[i].copy(), action[i])
                    if by_name:
                        item += (heads[i].copy() if i in heads else None,)
                    if use_open:
                        item += (int(on_group[i]),)
                    if marks is not None:
                        item += (marks[i],)
                    if auto:
                        item += (au[k].copy(),)
                    if sam:
                        qs = int(au[k]["skip"]) if auto else skip
                        item += (dict(events=se.events(slots[i]) if mapped(rows[i]) else None, qstart=qs, qend=qs + int(info[i]["q_events"]), map=maps[per * k],
                                      cand_maps=maps[per * k + 1:per * k + 5] if candidates else None),)
                    yield item
                se.reset(d_slots)
            tick_now = sch.tick
            held = sch.end_tick(reason, line, src, action, on_group if book is not None else None, None if marks is None else [m and (m["tt"], m["tv"]) for m in marks])
            if cover is not None:  # one call for the tick; the new mask holds from the next tick on
                covered = [(int(rows[i]["rid"]), int(rows[i]["pos_st"]), int(rows[i]["pos_end"])) for i in decided
                           if line[i] and action[i] == "A" and 0 <= int(rows[i]["pos_st"]) < int(rows[i]["pos_end"])]
                if covered:
                    cover["open"] = se.add_coverage(covered)
                    cover["intervals"] += len(covered)
                    cover["bases"] += sum(e - b for _, b, e in covered)
                    if trace is not None:
                        trace.append(f"tick {tick_now} cover n={len(covered)} open={cover['open']}")
            if gcover is not None:  # one add for the tick, then how deep every group is; the live table holds from the next tick on
                covered = [(int(rows[i]["rid"]), int(rows[i]["pos_st"]), int(rows[i]["pos_end"])) for i in decided
                           if line[i] and action[i] == "A" and 0 <= int(rows[i]["pos_st"]) < int(rows[i]["pos_end"])]
                if covered:
                    n_open = se.add_coverage(covered)
                    gcover["intervals"] += len(covered)
                    gcover["bases"] += sum(e - b for _, b, e in covered)
                    if trace is not None:
                        trace.append(f"tick {tick_now} cover n={len(covered)} open={n_open}")
                    gcover["records"] = se.group_coverage()
                    for g, name in enumerate(group_names):
                        if g not in gcover["full"] and group_is_full(int(gcover["records"][g]["columns"]), int(gcover["records"][g]["capped"])):
                            gcover["full"].add(g)
                            if trace is not None:
                                trace.append(f"tick {tick_now} full group={name}")
            if marks is not None:
                for i in decided:
                    note_truth(account, marks[i]["tt"], marks[i]["edge"], action[i], marks[i]["tv"], sch_sent[i], held[i], marks[i]["length"])
            if book is not None and summary is not None:
                for g, at in enumerate(sch.closed_at):
                    if at >= 0:
                        summary[("closed_at", g)] = at
            if summary is not None and targets is not None:
                for i, why in enumerate(reason):
                    if why:
                        n = summary.setdefault(action[i], [0, 0])
                        n[0] += 1
                        n[1] += sch_sent[i] + held[i]
    finally:
        if own:
            se.close()


def _map_or_none(m):
    """a row's slice of Session.event_maps: None when the row has no map (not mapped, or the library wrote nothing for it)"""
    return m.copy() if len(m) and m[0, 0] != np.iinfo(np.int32).min else None


def class_of_decision(decision, mode):
    """the class a decision stands for: 'T' on target, 'O' off target, 'N' none (decision: api.target_decide's 'A', 'U' or None)"""
    return "N" if decision is None else ("T" if (decision == "A") == (mode == api.ENRICH) else "O")


def target_tags(cls, mode, min_events, margin):
    """tc:A:<T|O|N> ac:A:<A|U|P> tm:f:<(other - mine) / n_events> for a CLASS_DTYPE record at a decision: the target class (N: no
    class decision), the action (P: the read proceeds) and the per-event margin it had -- mine is the on-target score under
    ENRICH and the off-target score under DEPLETE; nan when it is undefined (both classes empty, no events)."""
    dec = api.target_decide(cls, mode, min_events, margin)
    tc = class_of_decision(dec, mode)
    on, off, n = float(cls["on_score"]), float(cls["off_score"]), int(cls["n_events"])
    mine, other = (on, off) if mode == api.ENRICH else (off, on)
    with np.errstate(all="ignore"):
        tm = float(np.float64(other) - np.float64(mine)) / n if n > 0 else float("nan")
    return f"\ttc:A:{tc}\tac:A:{dec or 'P'}\ttm:f:{'nan' if tm != tm else '%.4f' % tm}"


def group_tags(head, names):
    """tg:Z:<name of the best entry, * for the background> gm:f:<(second - best) / n_events> for a GROUP_HEAD_DTYPE record at a
    decision (replay::group_tags): a missing runner-up counts as +inf; nan where undefined (no events, no best entry, +inf
    against +inf)."""
    best, second, n = int(head["best"]), int(head["second"]), int(head["n_events"])
    name = names[best] if 0 <= best < len(names) else "*"
    runner = float("inf") if second < 0 else float(head["second_score"])
    with np.errstate(all="ignore"):
        gm = float((np.float64(runner) - np.float64(float(head["best_score"]))) / n) if n > 0 and best >= 0 else float("nan")
    return f"\ttg:Z:{name}\tgm:f:{'nan' if gm != gm else '%.4f' % gm}"


def quota_tags(on_group, names):
    """og:Z:<name of the open-class record's on_group, * for none> (replay::quota_tags)"""
    return "\tog:Z:" + (names[on_group] if 0 <= on_group < len(names) else "*")


def truth_tags(marks, names=None):
    """tt:A:<true class T|O, N: the read has no truth> tv:A:<verdict of the line's tc: C|W|N> for the truth dict of a replay item
    (replay::truth_tags); with names (by_name) also tn:Z:<the true group's name, * for the background, . for a read without truth>
    gv:A:<verdict of the line's tg> (replay::truth_group_tags)."""
    out = f"\ttt:A:{marks['tt']}\ttv:A:{marks['tv']}"
    if names is not None:
        g = marks["true_group"]
        out += "\ttn:Z:" + ("." if g is None or g < 0 else (names[g] if g < len(names) else "*")) + f"\tgv:A:{marks['gv']}"
    return out


def new_truth_account(groups=False):
    """the account of a replay with truth= (the twin of truth_rules.hpp's TruthAccount; integer sums only): per true class reads,
    samples sent / held / in the file, edge reads, counts by action and by verdict; with groups the group verdicts"""
    acc = {c: dict(reads=0, sent=0, held=0, file=0, edge=0, A=0, U=0, P=0, C=0, W=0, N=0) for c in "TON"}
    acc["groups"] = dict(C=0, W=0, N=0) if groups else None
    return acc


def note_truth(account, tt, edge, action, tv, sent, held, in_file):
    """TruthAccount::note: one decided read"""
    c = account[tt if tt in ("T", "O") else "N"]
    c["reads"] += 1
    c["sent"] += int(sent)
    c["held"] += int(held)
    c["file"] += int(in_file)
    c["edge"] += int(bool(edge))
    c[action if action in ("A", "U") else "P"] += 1
    c[tv if tv in ("C", "W") else "N"] += 1


def truth_enrichment(account):
    """((on-target sequenced, all sequenced), (on-target in the file, all in the file), enrichment by signal or None) over the reads
    that have truth; sequenced = sent + held.  The ratio is formed only when neither divisor is 0 (TruthAccount::format)."""
    seq = [account[c]["sent"] + account[c]["held"] for c in "TO"]
    fil = [account[c]["file"] for c in "TO"]
    ok = sum(seq) > 0 and fil[0] > 0
    return (seq[0], sum(seq)), (fil[0], sum(fil)), (float(seq[0]) * float(sum(fil))) / (float(sum(seq)) * float(fil[0])) if ok else None


def format_truth_summary(account):
    """the `truth:` lines `sigfish-amd realtime --truth` ends its stderr with (TruthAccount::format), from summary["truth"]"""
    out = ""
    for k in "TON":
        c = account[k]
        out += ("[realtime] truth: %s reads=%d sent=%d held=%d file=%d A=%d U=%d P=%d C=%d W=%d N=%d edge=%d\n"
                % (k, c["reads"], c["sent"], c["held"], c["file"], c["A"], c["U"], c["P"], c["C"], c["W"], c["N"], c["edge"]))
    if account["groups"] is not None:
        out += "[realtime] truth: groups C=%d W=%d N=%d\n" % (account["groups"]["C"], account["groups"]["W"], account["groups"]["N"])
    (s_on, s_all), (f_on, f_all), ratio = truth_enrichment(account)
    quotient = lambda a, b: "%.4f" % (float(a) / float(b)) if b > 0 else "-"
    return out + ("[realtime] truth: on-target share of the sequenced samples (sent + held) %d / %d = %s, of the file's samples %d / %d = %s, enrichment by signal %s\n"
                  % (s_on, s_all, quotient(s_on, s_all), f_on, f_all, quotient(f_on, f_all), "-" if ratio is None else "%.4f" % ratio))


def format_group_summary(summary, names):
    """the lines `sigfish-amd realtime --by-name` ends its stderr with: accepted reads per best entry, the background last; with a
    quota (summary["quota"]) the named groups' lines gain quota=N closed_at=<tick, - for a group still open>"""
    quota = summary.get("quota", 0)
    tail = lambda g: " quota=%d closed_at=%s" % (quota, summary.get(("closed_at", g), "-")) if quota and g < len(names) else ""
    return "".join("[realtime] group %s: accepted %d reads%s\n" % (names[g] if g < len(names) else "*", summary.get(("group", g), 0), tail(g)) for g in range(len(names) + 1))


def group_is_full(columns, capped):
    """replay::group_is_full: every column of the group is capped; a group without columns is never full"""
    return columns > 0 and capped == columns


def group_cover_line(name, columns, capped, depth_sum):
    """replay::group_cover_line: a named group's line of the summary; `-` for a group without columns (the quotient is not formed)"""
    mean = "%.3f" % (int(depth_sum) / int(columns)) if columns > 0 else "-"
    return "[realtime] group depth %s\tcolumns=%d capped=%d mean_depth=%s\n" % (name, columns if columns > 0 else 0, capped if columns > 0 else 0, mean)


def format_group_cover_summary(summary, names):
    """the lines `sigfish-amd realtime --group-cap` adds to its stderr, from summary["group_cover"]"""
    c = summary["group_cover"]
    return "[realtime] group cap %d\t%d intervals, %d bases added\n" % (c["cap"], c["intervals"], c["bases"]) + "".join(
        group_cover_line(n, int(c["records"][g]["columns"]), int(c["records"][g]["capped"]), int(c["records"][g]["depth_sum"])) for g, n in enumerate(names))


def format_reach_summary(summary):
    """the line `sigfish-amd realtime --lead` adds to its stderr, from summary["reach"]"""
    c = summary["reach"]
    return "[realtime] reach: lead %d%s\ton-target columns: %d\n" % (c["lead"], ", stranded" if c["stranded"] else "", c["columns"])


def format_reach_group_summary(summary):
    """the line `sigfish-amd realtime --group-lead` adds to its stderr, from summary["reach_groups"] (the twin of replay.hpp's reach_group_line)"""
    c = summary["reach_groups"]
    return "[realtime] reach groups: lead %d%s\tlabelled columns: %d\n" % (c["lead"], ", stranded" if c["stranded"] else "", c["columns"])


def format_cover_summary(summary):
    """the line `sigfish-amd realtime --depth-cap` adds to its stderr, from summary["cover"]"""
    c = summary["cover"]
    return "[realtime] coverage: cap %d\t%d intervals, %d bases added\topen target columns at the end: %d of %d\n" % (c["cap"], c["intervals"], c["bases"], c["open"], c["base"])


def format_summary(summary):
    """the line `sigfish-amd realtime --targets` ends its stderr with, from the dict replay(summary=) filled"""
    get = lambda a: summary.get(a, [0, 0])
    return ("[realtime] targets: accepted (A) %d reads, %d samples\tunblocked (U) %d reads, %d samples\tproceeded (P) %d reads, %d samples (sent + held)\n"
            % (*get("A"), *get("U"), *get("P")))


def auto_tags(auto):
    """qs:i:<skip> as:A:<P|E|F> for a SESSION_AUTO_DTYPE record: found at a mid-read point, found at the final point, fallback"""
    st = int(auto["status"])
    how = "F" if (st & 15) != api.AUTO_RESOLVED else ("E" if st & api.AUTO_AT_FINAL else "P")
    return f"\tqs:i:{int(auto['skip'])}\tas:A:{how}"


def format_line(read_id, n_samples, names, seq_lengths, row, info, span, reason, auto=None, target=None, group=None, quota=None, truth=None):
    """The line `sigfish-amd realtime` prints for a decision, or "" when its row is not mapped: paf_row (query_size as dtw passes
    it, last query event - first), then ne:i:<query events> ns:i:<samples sent> dc:A:<reason>.  n_samples: of the whole read.
    auto: the decision's automatic start (replay with skip = -1): qs:i and as:A follow the three tags.
    target: (class record, mode, min_events, margin) of a replay with targets=: target_tags() follow.
    group: (head record, group names) of a replay with by_name=True: group_tags() follow those.
    quota: (on_group, group names) of a replay with quota=: quota_tags() follows those.
    truth: (truth dict, group names or None) of a replay with truth=: truth_tags() follow all others."""
    if not mapped(row):
        return ""
    rid = int(row["rid"])
    base = api.paf_row(row, read_id, names[rid], span[0], span[1], int(info["q_events"]) - 1, int(n_samples), int(seq_lengths[rid]))
    tail = ("" if auto is None else auto_tags(auto)) + ("" if target is None else target_tags(*target)) + ("" if group is None else group_tags(*group)) + ("" if quota is None else quota_tags(*quota)) + ("" if truth is None else truth_tags(*truth))
    return f"{base[:-1]}\tne:i:{int(info['q_events'])}\tns:i:{int(info['n_samples'])}\tdc:A:{reason}{tail}\n"


def format_candidates(read_id, n_samples, names, seq_lengths, row, cand, info, span, reason, target=None, group=None, quota=None, truth=None):
    """The candidate lines that follow a decision's primary line under --candidates: one per valid row of `cand`, best first, each
    the tp:A:S line of paf_row_ex with the primary's span and query_size and the primary's three tags; "" when the primary has no
    line."""
    if not mapped(row):
        return ""
    out = []
    for r in cand:
        if not mapped(r):
            continue
        rid = int(r["rid"])
        base = api.paf_row(r, read_id, names[rid], span[0], span[1], int(info["q_events"]) - 1, int(n_samples), int(seq_lengths[rid]), tp="S")
        out.append(f"{base[:-1]}\tne:i:{int(info['q_events'])}\tns:i:{int(info['n_samples'])}\tdc:A:{reason}{'' if target is None else target_tags(*target)}{'' if group is None else group_tags(*group)}{'' if quota is None else quota_tags(*quota)}{'' if truth is None else truth_tags(*truth)}\n")
    return "".join(out)


def format_sam_line(read_id, names, row, info, reason, events, qstart, qend, pairs, flag, secondary=False, auto=None):
    """The SAM record of a decision's row in place of format_line's PAF line: api.sam_row_from_map over the slot's events
    [qstart, qend) and the row's event map, then the same ne:i / ns:i / dc:A tags (and qs:i / as:A with auto=).  "" when the row is
    not mapped, has no map, or sam_row_from_map refuses the map (RNA: a last reference column without a query event -- the ss
    string cannot express it; `dtw --sam` leaves such rows out too and counts them)."""
    if not mapped(row) or pairs is None or len(pairs) == 0:
        return ""
    try:
        base = api.sam_row_from_map(row, read_id, names[int(row["rid"])], events, qstart, qend, pairs, flag, secondary)
    except api.SfaError:
        return ""
    return f"{base[:-1]}\tne:i:{int(info['q_events'])}\tns:i:{int(info['n_samples'])}\tdc:A:{reason}{'' if auto is None else auto_tags(auto)}\n"


def format_sam(read_id, names, row, info, reason, sam, flag, cand=None, auto=None):
    """(text, refused) for one item of replay(sam=True): the primary's record and, with cand= (the item's candidates), the records
    of its valid candidates behind it, best first, as secondaries (FLAG | 256); `sam` is the item's last element.  refused: mapped
    rows left out because they have no printable map.  ("", 0) when the primary is not mapped: a decision without a line."""
    if not mapped(row):
        return "", 0
    out, refused = [], 0
    todo = [(row, sam["map"], False)] + ([(r, m, True) for r, m in zip(cand, sam["cand_maps"]) if mapped(r)] if cand is not None else [])
    for r, m, secondary in todo:
        line = format_sam_line(read_id, names, r, info, reason, sam["events"], sam["qstart"], sam["qend"], m, flag, secondary, None if secondary else auto)
        out.append(line)
        refused += line == ""
    return "".join(out), refused
