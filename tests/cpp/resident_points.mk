# test_resident_points: the host mirror's SearchLocalPoints / FuseSearch over ResidentPoints next to the staged mirror
# calls, on the cases tests/test_gpu_resident_points_mirror.py writes (GPU).  make -f resident_points.mk
CXX ?= g++
PKG = ../../orb-slam-birdview_amd
HOSTH = $(wildcard $(PKG)/host/*.h)

test_resident_points: test_resident_points.cc $(HOSTH) $(PKG)/liborbslam_host.so $(PKG)/liborbgpu.so
	$(CXX) -O2 -std=c++17 -Wall -o $@ test_resident_points.cc -L$(PKG) -lorbslam_host -lorbgpu -Wl,-rpath,'$$ORIGIN/$(PKG)'

clean:
	rm -f test_resident_points
.PHONY: clean
