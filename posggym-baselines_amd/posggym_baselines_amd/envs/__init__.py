"""Environment models the GPU engine implements (Driving-v1, PursuitEvasion-v1,
CooperativeReaching-v0, PredatorPrey-v0) and the recognition of a posggym-style ``env.model``."""
from posggym_baselines_amd.envs.driving import (  # noqa: F401
    GRIDS,
    DrivingModel,
    pack_obs,
    unpack_obs,
)
from posggym_baselines_amd.envs.cooperative_reaching import CooperativeReachingModel  # noqa: F401
from posggym_baselines_amd.envs.predator_prey import PredatorPreyModel  # noqa: F401
from posggym_baselines_amd.envs.pursuit_evasion import PursuitEvasionModel  # noqa: F401

# posggym registrations the engine restates, with the env kwargs each accepts
# and their posggym defaults (the reference's experiments: Driving-v1
# "14x14RoundAbout", PursuitEvasion-v1 "16x16", baseline_exps/exp_utils.py)
_SUPPORTED = {
    "Driving-v1": (DrivingModel, {"grid": "14x14RoundAbout", "num_agents": 2,
                                  "obs_dim": (3, 1, 1)}),
    "PursuitEvasion-v1": (PursuitEvasionModel, {"grid": "16x16", "max_obs_distance": 12,
                                                "use_progress_reward": True}),
    # (size 3..8; mode "original" and num_goals 4 only: the model's constructor
    # raises NotImplementedError for anything else)
    "CooperativeReaching-v0": (CooperativeReachingModel, {"size": 5, "num_goals": 4,
                                                          "mode": "original",
                                                          "obs_distance": None}),
    # (open grids "5x5" and "10x10", two predators, cooperative only: the model's
    # constructor raises NotImplementedError for anything else)
    "PredatorPrey-v0": (PredatorPreyModel, {"grid": "10x10", "num_predators": 2, "num_prey": 3,
                                            "cooperative": True, "prey_strength": None,
                                            "obs_dim": 2}),
}
# posggym env kwargs that do not change the generative model
_IGNORED_KWARGS = {"render_mode", "max_episode_steps"}
# kwargs the restatements implement at one value only: accepted at that value,
# anything else raises (PursuitEvasion-v1 always divides its rewards by the
# normaliser, pursuit_evasion.py reward_norm; a planner built for
# normalize_reward=False would silently plan with other rewards)
_FIXED_KWARGS = {"normalize_reward": True}


def engine_model(model):
    """The engine-side model for ``model``: the builder's own models as they are;
    a posggym-style model (``model.spec.id`` + ``model.spec.kwargs``, e.g. the
    ``env.model`` the reference's planners receive) is mapped to the engine's
    restatement of that registration.  Anything else raises
    ``NotImplementedError`` -- the engine has no generic (Python) model path."""
    if hasattr(model, "configure_engine"):
        return model
    spec = getattr(model, "spec", None)
    env_id = getattr(spec, "id", None)
    if env_id not in _SUPPORTED:
        raise NotImplementedError(
            f"no GPU generative model for {env_id or type(model).__name__}; the engine "
            f"implements {sorted(_SUPPORTED)}")
    cls, defaults = _SUPPORTED[env_id]
    kwargs = dict(getattr(spec, "kwargs", None) or {})
    for k in _IGNORED_KWARGS:
        kwargs.pop(k, None)
    for k, v in _FIXED_KWARGS.items():
        if k in kwargs:
            if kwargs.pop(k) != v:
                raise NotImplementedError(f"{env_id}: {k}={not v} is not restated (only {v})")
    unknown = set(kwargs) - set(defaults)
    if unknown:
        raise NotImplementedError(f"{env_id}: unsupported env kwargs {sorted(unknown)}")
    args = dict(defaults, **kwargs)
    if "obs_dim" in args and env_id != "PredatorPrey-v0":    # (Driving-v1's triple; PredatorPrey's is an int)
        args["obs_dim"] = tuple(args["obs_dim"])
    if isinstance(args.get("grid"), str) and args["grid"] not in GRIDS and \
            env_id == "Driving-v1":
        raise NotImplementedError(f"Driving-v1 grid {args['grid']!r} is not restated")
    try:
        return cls(**args)
    except KeyError as e:
        raise NotImplementedError(f"{env_id}: grid {e} is not restated") from None
