// edge_network.h -- the selection network of the edge measure (mvs_kernels.h edge_pixel) as an X-macro.  No HIP in here: a host program expands the
// same list over bit lanes and checks it (tests/cpp/edge_network_check.cpp, the zero-one principle over all 2^25 inputs).
//
// DR_EDGE_NETWORK(CE) expands to CE(a, b) for each comparator, in order; CE(a, b) leaves min(v[a], v[b]) in v[a] and the max in v[b], a < b.
// After the network, wire DR_EDGE_WIRE of the 25 holds the DR_EDGE_WIRE + 1 = 15th smallest input (k = 15, 1-based: module.py:1336,1343).
// Knuth's merge exchange (TAOCP 5.2.2 M) for 25 inputs has 138 comparators; the DR_EDGE_COMPARATORS = 113 below are the ones element 14 of the sorted
// order depends on.
#pragma once

#define DR_EDGE_INPUTS 25
#define DR_EDGE_WIRE 14
#define DR_EDGE_COMPARATORS 113

#define DR_EDGE_NETWORK(CE) \
  CE(0,16) CE(1,17) CE(2,18) CE(3,19) CE(4,20) CE(5,21) CE(6,22) CE(7,23) CE(8,24) CE(0,8) CE(1,9) CE(2,10) \
  CE(3,11) CE(4,12) CE(5,13) CE(6,14) CE(7,15) CE(16,24) CE(8,16) CE(9,17) CE(10,18) CE(11,19) CE(12,20) CE(13,21) \
  CE(14,22) CE(15,23) CE(0,4) CE(1,5) CE(2,6) CE(3,7) CE(8,12) CE(9,13) CE(10,14) CE(11,15) CE(16,20) CE(17,21) \
  CE(18,22) CE(19,23) CE(4,16) CE(5,17) CE(6,18) CE(7,19) CE(12,24) CE(4,8) CE(5,9) CE(6,10) CE(7,11) CE(12,16) \
  CE(13,17) CE(14,18) CE(15,19) CE(20,24) CE(0,2) CE(1,3) CE(4,6) CE(5,7) CE(8,10) CE(9,11) CE(12,14) CE(13,15) \
  CE(16,18) CE(17,19) CE(20,22) CE(21,23) CE(2,16) CE(3,17) CE(6,20) CE(7,21) CE(10,24) CE(2,8) CE(3,9) CE(6,12) \
  CE(7,13) CE(10,16) CE(11,17) CE(14,20) CE(15,21) CE(18,24) CE(2,4) CE(3,5) CE(6,8) CE(7,9) CE(10,12) CE(11,13) \
  CE(14,16) CE(15,17) CE(18,20) CE(19,21) CE(22,24) CE(0,1) CE(2,3) CE(4,5) CE(6,7) CE(8,9) CE(10,11) CE(12,13) \
  CE(14,15) CE(16,17) CE(18,19) CE(20,21) CE(22,23) CE(1,16) CE(3,18) CE(5,20) CE(7,22) CE(9,24) CE(7,14) CE(9,16) \
  CE(11,18) CE(13,20) CE(11,14) CE(13,16) CE(13,14)
