"""Mirror of the reference's optimizer/ package: the particle swarm of optimizer/pso.py on the device (csrc/pso.hip)."""
from .pso import ParticleSwarmOptimizer, SwarmState, pso_draws  # noqa: F401
