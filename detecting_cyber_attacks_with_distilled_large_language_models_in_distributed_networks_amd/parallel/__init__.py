"""Distribution: process groups (RCCL/gloo), FedAvg collectives, launcher, TCP compat transport."""
from .comm import DistInfo, barrier, init_distributed, shutdown  # noqa: F401
from .fedavg import aggregate_state_dicts, broadcast_model, fedavg_  # noqa: F401
from .robust import RobustAggregator, make_robust, robust_aggregate_  # noqa: F401
from .robust_dist import robust_dist_aggregate_  # noqa: F401
from .server_opt import ServerOptimizer, make_server_optimizer  # noqa: F401
