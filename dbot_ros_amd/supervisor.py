"""Track supervisor: the loop the reference leaves to a person.  Its controller shows a found pose in rviz and waits
for a click before it starts the tracker (R:source/dbot_ros/tracker/object_tracker_controller_service_node.cpp:180-195),
and nothing tells a running tracker that its object is gone.  TrackSupervisor judges every estimate against its frame
(dbot_ros_amd/assess.py), counts the frames that read LOST, and -- given a finder -- re-initialises the tracker from a
found pose that the assessor confirms.  Host logic only: the tracker, the assessor and the finder do the device work.
"""
import numpy as np

from .assess import CONTOUR_ABSENT, CONTOUR_PRESENT, LOST, OCCLUDED, SUPPORTED


class TrackSupervisor:
    """TrackSupervisor(tracker, assessor, find=None, lost_frames=3, occluded_frames=0, find_bodies=None).step(frame) ->
    (estimate, verdicts [parts], event).

    tracker   .track(frame) -> State, .initialize([state]), .parts; driven frame by frame only.
    assessor  .assess_state(tracker, state, frame) -> Assessment of one pose (a PoseAssessor).
    find      None, or find(frame) -> a State (parts*12) or None; one object only.
    A frame counts as lost when any body reads LOST, and -- with occluded_frames > 0 -- when any body has read OCCLUDED
    for more than occluded_frames consecutive frames.  The lost_frames-th such frame in a row has the event "lost".
    Without a finder the event repeats every further lost_frames such frames.  With a finder the next frame that still
    counts as lost is searched: the found state is assessed against that frame, a SUPPORTED one re-initialises the
    tracker ("reacquired", and the returned estimate is the found state); no state or any other verdict is
    "find_failed", and the next attempt comes after another lost_frames such frames.  A frame that does not count as
    lost ends the run.  Other frames: event None.
    With the assessor's contour rule on (PoseAssessor(contour=...)) a found state must pass Assessment.confirmed_mask():
    SUPPORTED and its silhouette PRESENT.  contour_lost=True (it needs that rule) also counts a frame as lost when a
    body's contour verdict is ABSENT.
    find_bodies  None, or find_bodies(frame, lost [parts] bool, estimate) -> a State (parts*12) or None, for any number of
    parts (a SceneFinder: dbot_ros_amd/finder.py): in place of `find`, at the same moments.  `lost` names the bodies that
    make the frame count as lost (LOST, OCCLUDED for too long, or -- with contour_lost -- a silhouette that reads ABSENT);
    only those are to be searched, the others keep the estimate's poses.  The found state is confirmed on the searched
    bodies alone: each SUPPORTED (and PRESENT with the contour rule on); the others' verdicts do not count.  `find` and its
    one-object limit stay as they are; both at once: ValueError.
    refine    None, or a PoseRefiner over the tracker's sensor (.refine_state(tracker, state, frame) -> (State, record)): a
    found state is refined against the frame before it is confirmed, and the refined state is what the assessor judges
    and what re-initialises the tracker (`last_refinement`: its record).  With find_bodies every body is refined in the one
    call -- the refiner moves all bodies of a pose, so the searched bodies' ownership is taken against neighbours that
    move with them, and `last_refinement` reports every body -- but only the searched bodies take their refined pose: the
    others go on from the state find_bodies returned, bit for bit.  None: every step is what it was without."""

    def __init__(self, tracker, assessor, find=None, lost_frames=3, occluded_frames=0, look_ahead=False, contour_lost=False,
                 find_bodies=None, refine=None):
        if look_ahead:
            raise ValueError("TrackSupervisor drives the tracker frame by frame: a verdict decides what the next frame starts from")
        if int(lost_frames) < 1 or int(occluded_frames) < 0:
            raise ValueError("TrackSupervisor: lost_frames >= 1 and occluded_frames >= 0")
        self.tracker, self.assessor, self.find = tracker, assessor, find
        self.parts = int(tracker.parts)
        if find is not None and self.parts != 1:
            raise ValueError("TrackSupervisor: a finder searches for one object; this tracker has %d" % self.parts)
        if find is not None and find_bodies is not None:
            raise ValueError("TrackSupervisor: find and find_bodies are alternatives")
        self.find_bodies = find_bodies
        self.refine = refine
        self.last_refinement = None                         # the record of the last refined re-found state
        self.lost_frames, self.occluded_frames = int(lost_frames), int(occluded_frames)
        self.contour_lost = bool(contour_lost)
        if self.contour_lost and getattr(assessor, "contour", None) is None:
            raise ValueError("TrackSupervisor: contour_lost needs an assessor with the contour rule on")
        self.lost_run = 0                                   # consecutive frames that count as lost
        self.occluded_run = np.zeros(self.parts, dtype=int)  # consecutive OCCLUDED frames per body
        self.next_attempt = None                            # finder: the lost_run at which the next search comes (None: not lost)
        self.last = None                                    # the last frame's Assessment

    def reset(self):
        self.lost_run = 0
        self.occluded_run[:] = 0
        self.next_attempt = None

    def step(self, frame):
        if getattr(self.tracker, "_in_flight", 0) > 0:
            raise ValueError("TrackSupervisor.step: the tracker has frames in flight (submit / result); collect them first")
        est = self.tracker.track(frame)
        self.last = self.assessor.assess_state(self.tracker, est, frame)
        verdicts = np.asarray(self.last.verdicts).reshape(-1)[:self.parts].copy()
        self.occluded_run = np.where(verdicts == OCCLUDED, self.occluded_run + 1, 0)
        lost_bodies = verdicts == LOST                       # the bodies that make this frame count as lost
        if self.occluded_frames > 0:
            lost_bodies = lost_bodies | (self.occluded_run > self.occluded_frames)
        if self.contour_lost:
            lost_bodies = lost_bodies | (np.asarray(self.last.contour_verdicts).reshape(-1)[:self.parts] == CONTOUR_ABSENT)
        lost = bool(lost_bodies.any())
        if not lost:
            self.lost_run, self.next_attempt = 0, None
            return est, verdicts, None
        self.lost_run += 1
        if self.find is None and self.find_bodies is None:
            return est, verdicts, "lost" if self.lost_run % self.lost_frames == 0 else None
        if self.next_attempt is None:
            if self.lost_run < self.lost_frames:
                return est, verdicts, None
            self.next_attempt = self.lost_run + 1
            return est, verdicts, "lost"
        if self.lost_run < self.next_attempt:
            return est, verdicts, None
        self.next_attempt = self.lost_run + self.lost_frames
        state = self.find(frame) if self.find is not None else self.find_bodies(frame, lost_bodies.copy(), est)
        if state is None:
            return est, verdicts, "find_failed"
        state = np.asarray(state, dtype=np.float64).reshape(-1)
        if self.refine is not None:
            given = state
            state, self.last_refinement = self.refine.refine_state(self.tracker, state, frame)
            state = np.array(state, dtype=np.float64).reshape(-1)
            if self.find_bodies is not None:   # only the searched bodies take the refined pose: the others keep theirs, bit for bit
                keep = np.repeat(~lost_bodies, len(state) // self.parts)
                state[keep] = given[keep]
        found = self.assessor.assess_state(self.tracker, state, frame)
        if self.find is not None:
            ok = bool((np.asarray(found.verdicts).reshape(-1) == SUPPORTED).all())
            if getattr(found, "contour_verdicts", None) is not None:
                ok = bool(found.confirmed_mask().all())
        else:   # only the searched bodies are confirmed
            ok = bool((np.asarray(found.verdicts).reshape(-1)[:self.parts][lost_bodies] == SUPPORTED).all())
            if getattr(found, "contour_verdicts", None) is not None:
                ok = ok and bool((np.asarray(found.contour_verdicts).reshape(-1)[:self.parts][lost_bodies] == CONTOUR_PRESENT).all())
        if not ok:
            return est, verdicts, "find_failed"
        self.tracker.initialize([state])
        self.reset()
        return state.copy(), verdicts, "reacquired"
