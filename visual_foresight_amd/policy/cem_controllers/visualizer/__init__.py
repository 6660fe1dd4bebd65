"""Plan visualisation of the CEM controllers (reference ``visual_mpc/policy/cem_controllers/visualizer``)."""
