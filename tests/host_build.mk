# The host build of a sensor's specification (csrc/<name>_core.h): the build that the device code must equal bit for bit.  Test
# infrastructure, included by tests/<name>_host/Makefile, which sets NAME and CHAIN (the sensors whose specifications <name>_core.h
# includes, itself last).  The flags live here alone: one edit changes what all four suites compare against.
CXX ?= g++
FMAFLAG := $(shell grep -q -w fma /proc/cpuinfo && echo -mfma)
CSRC = ../../hrl_pybullet_envs_amd/csrc
FLAGS = -std=c++17 -ffp-contract=off $(FMAFLAG) -DHRL_EMU
WARN = -Wall -Wno-unknown-pragmas
PLAIN = -O2 -fPIC $(FLAGS) $(WARN) -shared
SANITISED = -O1 -g $(FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined $(WARN)
HDRS = $(CHAIN:%=$(CSRC)/%_core.h) $(CSRC)/step_core.h $(CSRC)/host_cfg.h ../../include/hrl_envs.h $(CHAIN:%=../../include/hrl_%.h) check_cases.h ../check_main.h ../host_build.mk
all: lib$(NAME)_host.so $(NAME)_check_main
lib%_host.so: %_host.cpp second_unit.cpp $(HDRS)
	$(CXX) $(PLAIN) -o $@ $*_host.cpp second_unit.cpp -lm
# stand-alone and sanitised: run as a subprocess, never loaded into python
%_check_main: %_check_main.cpp second_unit.cpp $(HDRS)
	$(CXX) $(SANITISED) -o $@ $*_check_main.cpp second_unit.cpp -lm
clean:
	rm -f lib$(NAME)_host.so $(NAME)_check_main
