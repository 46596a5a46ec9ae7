// Control plane of the multi-rank engines (Llama pipeline, Llama tensor parallel, split
// UNet): a star of framed-TCP sockets on rank 0, carrying JSON.  Host code only (json.h,
// net.h), so the runtime self-test drives it with threads on loopback.
//
// open() is the rendezvous: every rank hands in a hello (the engines publish IPC handles
// as hex in it) and leaves with table(), every rank's hello indexed by rank.  After it
// the engines exchange their own commands over send()/recv()/fd(); barrier() and
// verdict() are the two collectives all of them need.
#pragma once

#include <chrono>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "json.h"
#include "net.h"

namespace cake {

inline void send_json(int fd, const Json& j) {
  const std::string t = j.dump();
  send_frame(fd, reinterpret_cast<const uint8_t*>(t.data()), (uint32_t)t.size());
}
inline Json recv_json(int fd) { return Json::parse(recv_frame(fd)); }

class Star {
 public:
  Star() = default;
  Star(const Star&) = delete;
  Star& operator=(const Star&) = delete;
  ~Star() { close(); }

  // Rank 0 listens on addr ("host:port") until ranks 1..world-1 have each said hello once,
  // then sends every rank the table; a hello whose rank is out of range or already seen
  // fails the start with `bad_hello`.  A worker tries to connect every 200 ms until
  // connect_timeout_s has passed, then rethrows the last connect error.
  void open(const std::string& addr, int rank, int world, const Json& hello,
            double connect_timeout_s, const char* bad_hello) {
    std::string host;
    int port = 0;
    split_host_port(addr, &host, &port);
    rank_ = rank;
    table_.assign(world, Json());
    if (rank == 0) {
      table_[0] = hello;
      fds_.assign(world - 1, -1);
      const int lfd = tcp_listen(host, port);
      int fd = -1;  // accepted, not yet in fds_
      try {
        for (int i = 1; i < world; ++i) {
          fd = tcp_accept(lfd, nullptr);
          tcp_set_timeout(fd, 0);
          const Json j = recv_json(fd);
          const int r = (int)j.get("rank").as_int();
          if (r < 1 || r >= world || fds_[r - 1] >= 0) throw std::runtime_error(bad_hello);
          table_[r] = j.get("hello");
          fds_[r - 1] = fd;
          fd = -1;
        }
      } catch (...) {
        tcp_close(fd);
        tcp_close(lfd);
        throw;
      }
      tcp_close(lfd);
      Json all = Json::array();
      for (const auto& t : table_) all.push(t);
      Json m = Json::object();
      m.set("table", all);
      broadcast(m);
    } else {
      const auto deadline =
          std::chrono::steady_clock::now() + std::chrono::duration<double>(connect_timeout_s);
      for (;;) {
        try {
          fds_.assign(1, tcp_connect(host, port, 2.0));
          break;
        } catch (const std::exception&) {
          if (std::chrono::steady_clock::now() > deadline) throw;
          std::this_thread::sleep_for(std::chrono::milliseconds(200));
        }
      }
      tcp_set_timeout(fds_[0], 0);
      Json m = Json::object();
      m.set("rank", Json::integer(rank));
      m.set("hello", hello);
      send(0, m);
      const Json t = recv(0);
      for (int r = 0; r < world; ++r) table_[r] = t.get("table").at(r);
    }
  }

  const std::vector<Json>& table() const { return table_; }

  // the socket to `peer`: on rank 0 a worker's rank (1..world-1), on a worker 0
  int fd(int peer) const { return fds_.at(rank_ == 0 ? peer - 1 : peer); }
  void send(int peer, const Json& j) const { send_json(fd(peer), j); }
  Json recv(int peer) const { return recv_json(fd(peer)); }
  // the ranks 1..workers() this rank is the hub of: world - 1 on rank 0, none on a worker
  int workers() const { return rank_ == 0 ? (int)fds_.size() : 0; }
  void broadcast(const Json& j) const {
    for (int r = 1; r <= workers(); ++r) send(r, j);
  }

  // every rank reaches this point, then every rank leaves it; any other message where
  // the barrier's is due means the control stream lost step, and throws
  void barrier() const {
    Json b = Json::object();
    b.set("cmd", Json::string("barrier"));
    auto take = [](int fd) {
      const Json j = recv_json(fd);
      if (!j.has("cmd") || j.get("cmd").as_string() != "barrier")
        throw std::runtime_error("control barrier: bad message");
    };
    if (rank_ == 0) {
      for (int fd : fds_) take(fd);
      broadcast(b);
    } else {
      send(0, b);
      take(fds_.at(0));
    }
  }

  // every rank hands in its complaint (empty: none); all of them return the first
  // non-empty one in rank order
  std::string verdict(const std::string& bad) const {
    Json m = Json::object();
    if (rank_ != 0) {
      m.set("bad", Json::string(bad));
      send(0, m);
      return recv(0).get("bad").as_string();
    }
    std::string first = bad;
    for (int fd : fds_) {
      const std::string s = recv_json(fd).get("bad").as_string();
      if (first.empty()) first = s;
    }
    m.set("bad", Json::string(first));
    broadcast(m);
    return first;
  }

  void close() {
    for (int fd : fds_) tcp_close(fd);
    fds_.clear();
  }

 private:
  int rank_ = 0;
  std::vector<int> fds_;  // rank 0: the sockets of ranks 1..world-1; a worker: the one to rank 0
  std::vector<Json> table_;
};

}  // namespace cake
