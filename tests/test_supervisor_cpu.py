"""The track supervisor's state machine (dbot_ros_amd/supervisor.py) driven with a fake tracker, assessor and finder:
no device."""
import numpy as np
import pytest

from dbot_ros_amd.assess import Assessment, LOST, OCCLUDED, OUT_OF_VIEW, SUPPORTED
from dbot_ros_amd.supervisor import TrackSupervisor


class FakeTracker:
    def __init__(self, parts=1):
        self.parts = parts
        self.frames, self.initialized = [], []
        self._in_flight = 0

    def track(self, frame):
        self.frames.append(frame)
        return np.full(self.parts * 12, float(frame))

    def initialize(self, states):
        self.initialized.append(np.array(states[0]))


class FakeAssessor:
    """Verdicts by script: script[frame] for the tracker's estimate, found[frame] for a found state (marked by 1000 + frame)."""

    def __init__(self, script, found=None):
        self.script, self.found, self.calls = script, found or {}, []

    def assess_state(self, tracker, state, frame):
        is_found = float(np.asarray(state).reshape(-1)[0]) >= 1000.0
        self.calls.append((frame, is_found))
        v = self.found[frame] if is_found else self.script[frame]
        v = np.atleast_1d(np.array(v, dtype=np.int32))
        return Assessment(np.zeros((1, v.size, 5), dtype=np.int32), v[None])


def run(sup, n):
    return [sup.step(k)[2] for k in range(n)]


S, L, O, V = SUPPORTED, LOST, OCCLUDED, OUT_OF_VIEW


def test_lost_needs_consecutive_frames_and_supported_resets_the_count():
    script = [S, L, L, S, L, L, L, L, L, L, S, L]
    sup = TrackSupervisor(FakeTracker(), FakeAssessor(script), lost_frames=3)
    events = run(sup, len(script))
    assert events == [None, None, None, None, None, None, "lost", None, None, "lost", None, None]
    assert sup.lost_run == 1


def test_step_returns_the_estimate_and_the_verdicts():
    sup = TrackSupervisor(FakeTracker(parts=2), FakeAssessor([[S, O], [S, L]]), lost_frames=1)
    est, v, ev = sup.step(0)
    assert est.shape == (24,) and (est == 0.0).all() and v.tolist() == [S, O] and ev is None
    est, v, ev = sup.step(1)
    assert (est == 1.0).all() and v.tolist() == [S, L] and ev == "lost"      # any body LOST counts
    assert sup.last.verdicts.tolist() == [[S, L]]


def test_occluded_and_out_of_view_do_not_count_unless_asked():
    script = [O] * 6 + [V] * 3
    assert run(TrackSupervisor(FakeTracker(), FakeAssessor(script), lost_frames=2), 9) == [None] * 9
    # occluded_frames = 2: the third consecutive OCCLUDED frame is the first that counts, two such frames make "lost"
    sup = TrackSupervisor(FakeTracker(), FakeAssessor(script), lost_frames=2, occluded_frames=2)
    assert run(sup, 9) == [None, None, None, "lost", None, "lost", None, None, None]
    assert sup.occluded_run.tolist() == [0] and sup.lost_run == 0
    # a per-body counter: body 1 occluded throughout, body 0 never
    sup = TrackSupervisor(FakeTracker(parts=2), FakeAssessor([[S, O]] * 4), lost_frames=1, occluded_frames=2)
    assert run(sup, 4) == [None, None, "lost", "lost"]
    assert sup.occluded_run.tolist() == [0, 4]


def test_reacquired_reinitialises_and_resets():
    script = [S, L, L, L, S, S]
    calls = []

    def find(frame):
        calls.append(frame)
        return np.full(12, 1000.0 + frame)

    trk = FakeTracker()
    asr = FakeAssessor(script, found={3: S})
    sup = TrackSupervisor(trk, asr, find=find, lost_frames=2)
    out = [sup.step(k) for k in range(len(script))]
    assert [o[2] for o in out] == [None, None, "lost", "reacquired", None, None]
    assert calls == [3]                                       # searched on the frame after "lost", once
    assert len(trk.initialized) == 1 and (trk.initialized[0] == 1003.0).all()
    assert (out[3][0] == 1003.0).all()                        # the found state is that frame's estimate
    assert out[3][1].tolist() == [L]                          # ... next to the verdict that made it necessary
    assert (3, True) in asr.calls                             # the found state was assessed against that frame
    assert sup.lost_run == 0 and sup.next_attempt is None


def test_find_failed_and_its_retry_spacing():
    script = [L] * 12
    calls = []

    def find(frame):
        calls.append(frame)
        return None if frame < 6 else np.full(12, 1000.0 + frame)

    trk = FakeTracker()
    asr = FakeAssessor(script, found={6: L, 9: S})
    sup = TrackSupervisor(trk, asr, find=find, lost_frames=3)
    events = run(sup, 12)
    #          0     1     2       3              4     5     6              7     8     9
    assert events[:10] == [None, None, "lost", "find_failed", None, None, "find_failed", None, None, "reacquired"]
    assert calls == [3, 6, 9]                                 # every lost_frames frames after a failure
    assert len(trk.initialized) == 1                          # an unsupported find (frame 6) starts nothing
    assert events[10:] == [None, None]                        # the count starts again after the re-initialisation
    assert sup.lost_run == 2


def test_a_good_frame_ends_the_search():
    script = [L, L, S, L, L, L]
    calls = []
    sup = TrackSupervisor(FakeTracker(), FakeAssessor(script), find=lambda f: calls.append(f), lost_frames=2)
    assert run(sup, 6) == [None, "lost", None, None, "lost", "find_failed"]
    assert calls == [5]


def test_refusals():
    with pytest.raises(ValueError, match="one object"):
        TrackSupervisor(FakeTracker(parts=2), FakeAssessor([]), find=lambda f: None)
    TrackSupervisor(FakeTracker(parts=2), FakeAssessor([]))   # reporting only: fine
    with pytest.raises(ValueError, match="frame by frame"):
        TrackSupervisor(FakeTracker(), FakeAssessor([]), look_ahead=True)
    with pytest.raises(ValueError):
        TrackSupervisor(FakeTracker(), FakeAssessor([]), lost_frames=0)
    trk = FakeTracker()
    sup = TrackSupervisor(trk, FakeAssessor([S]))
    trk._in_flight = 1
    with pytest.raises(ValueError, match="in flight"):
        sup.step(0)
    assert trk.frames == []


def test_supervised_replay_refuses_look_ahead_and_unknown_keys():
    from dbot_ros_amd import node
    with pytest.raises(ValueError, match="look_ahead"):
        node.replay_dataset_supervised({}, None, "", look_ahead=True)
    with pytest.raises(ValueError, match="supervisor/lost"):
        node.replay_dataset_supervised({"supervisor": {"lost": 3}}, None, "")
    with pytest.raises(ValueError, match="supervisor/assess/sigma"):
        node.replay_dataset_supervised({"supervisor": {"assess": {"sigma": 3}}}, None, "")


def test_trackers_refuse_to_assess_without_the_frame_in_flight():
    from dbot_ros_amd.tracker import ParticleTracker

    class T(ParticleTracker):
        def __init__(self):
            self.moving_average = None

    t = T()
    with pytest.raises(ValueError, match="no frame tracked"):
        t.assess(assessor=object())
    t.moving_average = np.zeros(12)
    t._in_flight = 1
    with pytest.raises(ValueError, match="in flight"):
        t.assess(assessor=object())
