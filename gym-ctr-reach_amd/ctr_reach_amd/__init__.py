"""ctr_reach_amd -- MI355X-native batched concentric-tube-robot reach environment.

Drop-in for keshaviyengar/gym-ctr-reach's ``CTR-Reach-v0`` hot path (FK + step + reset),
with the environments stepped in lockstep by hand-written HIP kernels on gfx950.

  CtrReachVecEnv   N envs on one GPU, torch device tensors, one kernel launch per step
  CtrReachEnv      single-env facade with the reference's gym.GoalEnv surface
  Model            batched Model.forward_kinematics operator
  make             make('CTR-Reach-v0', **overrides)
  HerReplayBuffer  device HER replay feed (stable-baselines 2 'future' relabelling)
  MlpActor         the policy's actor, run by hand-written kernels (rollout, collect, follow)
  DdpgLearner      DDPG's critic and actor updates (forward, backward, Adam) on the device
  Td3Learner       the same with TD3's twin critics, both regressed in one pair of launches
  GaussianActor    SAC's tanh-Gaussian policy: an action and its log-probability in one launch
  SacLearner       SAC's policy step under twin critics with the learned temperature, on the device
  paths            line / circle / helix waypoint paths for follow() and dls_ik_path
"""
from .vec_env import CtrReachVecEnv, FollowResult  # noqa: F401
from .env import CtrReachEnv, Model, make  # noqa: F401
from .systems import Tube, default_kwargs, default_systems_parameters  # noqa: F401
from .goal_tolerance import GoalTolerance  # noqa: F401
from .ik import dls_ik_path, dls_ik_position_only  # noqa: F401
from .her import HerReplayBuffer  # noqa: F401
from .policy import GaussianActor, MlpActor, MlpCritic, TargetSmoothing, polyak_  # noqa: F401
from .learner import DdpgLearner, SacLearner, Td3Learner  # noqa: F401
from .paths import circle_path, helix_path, line_path  # noqa: F401
from . import paths  # noqa: F401
