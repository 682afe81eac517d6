# Top-level build.  Everything is compiled for gfx950 only.
#   lib   : dynamic_direct_lidar_odometry_amd/_lib/libddlo_gicp.so (the product: HIP kernels + C-ABI)
#   oracle: oracle/liboracle.so and oracle/_ref/libref_nanoflann.so (TEST-ONLY checker)
#   facade: tests/cpp/facade_replay (C++ NanoGICP facade driver, links the product)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := dynamic_direct_lidar_odometry_amd
CSRC := $(PKG)/csrc
LIBDIR := $(PKG)/_lib
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function
# the hot path, one file per stage (K1 .. K6), then the other translation units
STAGES := index_build covariance corr_search moments outputs
SRCS := $(STAGES) knn_tasks nftree cellgrid tietree cloud cellgrid_host align comm capi capi_debug preprocess voxel_order deskew odom segment seg_label seg_tracks seg_classes seg_project map track
# host-only translation units (.cpp), compiled as the others are so that they share runtime.hpp
HOST_SRCS := eval
OBJS := $(SRCS:%=$(LIBDIR)/%.o) $(HOST_SRCS:%=$(LIBDIR)/%.o)

all: lib oracle facade raycast

lib: $(LIBDIR)/libddlo_gicp.so

# every object from its .hip; the compiler writes the header dependencies (.d)
$(LIBDIR)/%.o: $(CSRC)/%.hip
	@mkdir -p $(@D)
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c $< -o $@

$(LIBDIR)/%.o: $(CSRC)/%.cpp
	@mkdir -p $(@D)
	$(HIPCC) $(HIPFLAGS) -x hip -MMD -MP -c $< -o $@

-include $(OBJS:.o=.d)

$(LIBDIR)/libddlo_gicp.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--no-undefined -o $@ $(OBJS)

oracle:
	$(MAKE) -C oracle

# test / bench infrastructure: the GPU twin of scene.py's ray caster (cfg 5 frame synthesis)
raycast: tools/raycast/libddlo_raycast.so

tools/raycast/libddlo_raycast.so: tools/raycast/raycast.hip
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

facade: tests/cpp/facade_replay

tests/cpp/facade_replay: tests/cpp/facade_replay.cpp include/nano_gicp/nano_gicp.hpp include/ddlo_gicp.h $(LIBDIR)/libddlo_gicp.so
	g++ -std=c++17 -O2 -Iinclude -o $@ tests/cpp/facade_replay.cpp -L$(LIBDIR) -lddlo_gicp -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

clean:
	rm -f $(LIBDIR)/*.o $(LIBDIR)/*.d $(LIBDIR)/*/*.o $(LIBDIR)/*/*.d $(LIBDIR)/*.so tests/cpp/facade_replay tools/raycast/libddlo_raycast.so
	$(MAKE) -C oracle clean

.PHONY: all lib oracle facade raycast clean

# Developer variants (load with DDLO_GICP_LIB): one stage file recompiled with a
# profile define, linked with the product's other objects.
#   lmprof    the LM step prints per-phase cycle counts
#   statsprof the search kernels fill the per-sub-group counters of gicp_debug_stats (tools/probe_tasks.py)
#   covprof   k_covariances2 stores per-group stamps (tools/cov_timeline.py)
# $(call VARIANT,name,defines,stage)
define VARIANT
$(LIBDIR)/$(1)/$(3).o: $(CSRC)/$(3).hip
	@mkdir -p $$(@D)
	$(HIPCC) $(HIPFLAGS) $(2) -MMD -MP -c $$< -o $$@
$(LIBDIR)/$(1)/libddlo_gicp.so: $(LIBDIR)/$(1)/$(3).o $(filter-out $(LIBDIR)/$(3).o,$(OBJS))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $$@ $$^
$(1): $(LIBDIR)/$(1)/libddlo_gicp.so
.PHONY: $(1)
-include $(LIBDIR)/$(1)/$(3).d
endef
$(eval $(call VARIANT,lmprof,-DDDLO_LM_PROF,moments))
$(eval $(call VARIANT,statsprof,-DDDLO_SEARCH_STATS,corr_search))
$(eval $(call VARIANT,covprof,-DDDLO_COV_PROF -DDDLO_DEV,covariance))

# development build: every file with the A/B environment knobs (devknobs.hpp) read
$(LIBDIR)/dev/%.o: $(CSRC)/%.hip
	@mkdir -p $(@D)
	$(HIPCC) $(HIPFLAGS) -DDDLO_DEV -MMD -MP -c $< -o $@
$(LIBDIR)/dev/%.o: $(CSRC)/%.cpp
	@mkdir -p $(@D)
	$(HIPCC) $(HIPFLAGS) -DDDLO_DEV -x hip -MMD -MP -c $< -o $@
$(LIBDIR)/dev/libddlo_gicp.so: $(SRCS:%=$(LIBDIR)/dev/%.o) $(HOST_SRCS:%=$(LIBDIR)/dev/%.o)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^
dev: $(LIBDIR)/dev/libddlo_gicp.so
.PHONY: dev
-include $(SRCS:%=$(LIBDIR)/dev/%.d) $(HOST_SRCS:%=$(LIBDIR)/dev/%.d)
